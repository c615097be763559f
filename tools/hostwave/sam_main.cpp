// The SAM kernels (svision_amd/csrc/svx_sam.hip) without a GPU: the phases of svx_sam_core.hpp -- the code the kernels run -- as loops
// over threads, tiles, lanes and waves.  Built with -fsanitize=address,undefined: the text lies in a heap block of exactly its bytes +
// the 64 bytes of slack include/svx.h asks for, the records in one of exactly their bytes; every read or write outside is reported.
// Build: g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// usage: sam_host TEXT NAMES OUT   TEXT: alignment lines; NAMES: the reference names in tid order, a line each.  OUT receives, little
//                                  endian: int64 n_lines, int64 line_off [n_lines + 1], int32 len tid pos flag span [n_lines] each,
//                                  int32 status, int64 the records' bytes, the records end to end (lines with len < 0 have none).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../svision_amd/csrc/svx_sam_core.hpp"

// the wave as svx_sam::record sees it: its lanes one after the other
struct Wave {
    template <class F> void each(F f) { for (uint32_t l = 0; l < svx_sam::WAVE; ++l) f(l); }
    template <class F> uint64_t ballot(F f) { uint64_t m = 0; for (uint32_t l = 0; l < svx_sam::WAVE; ++l) m |= (uint64_t)(f(l) ? 1 : 0) << l; return m; }
    template <class F> uint64_t sum(F f) { uint64_t v = 0; for (uint32_t l = 0; l < svx_sam::WAVE; ++l) v += f(l); return v; }
};

static std::vector<uint8_t> slurp(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<uint8_t> out;
    uint8_t buf[65536];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return out;
}

template <class T> static void put(FILE* f, const T* p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "write failed\n"); exit(2); } }

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: sam_host TEXT NAMES OUT\n"); return 2; }
    const std::vector<uint8_t> file = slurp(argv[1]), names_file = slurp(argv[2]);
    const uint64_t n = file.size();
    uint8_t* text = static_cast<uint8_t*>(malloc(n + svx_sam::SLACK));          // exactly the chunk and its slack
    if (n) memcpy(text, file.data(), n);
    memset(text + n, 0xA5, svx_sam::SLACK);
    // ---- the reference table, as the host builds it for the device
    std::vector<uint32_t> name_off(1, 0);
    std::vector<uint8_t> names;
    for (size_t p = 0; p < names_file.size();) {
        size_t q = p;
        while (q < names_file.size() && names_file[q] != '\n') ++q;
        names.insert(names.end(), names_file.begin() + p, names_file.begin() + q);
        name_off.push_back((uint32_t)names.size());
        p = q + 1;
    }
    const uint32_t n_ref = (uint32_t)name_off.size() - 1;
    std::vector<uint32_t> hash(n_ref);
    std::vector<int32_t> by_hash(n_ref);
    for (uint32_t t = 0; t < n_ref; ++t) {
        uint32_t h = 0x811C9DC5u;
        for (uint32_t k = name_off[t]; k < name_off[t + 1]; ++k) h = (h ^ names[k]) * 0x01000193u;
        hash[t] = h;
        by_hash[t] = (int32_t)t;
    }
    std::stable_sort(by_hash.begin(), by_hash.end(), [&](int32_t a, int32_t b) { return hash[a] < hash[b]; });
    std::vector<uint32_t> sorted_hash(n_ref);
    for (uint32_t k = 0; k < n_ref; ++k) sorted_hash[k] = hash[by_hash[k]];
    if (names.empty()) names.push_back(0);
    const svx_sam::RefTable rt{sorted_hash.data(), by_hash.data(), name_off.data(), names.data(), n_ref};
    // ---- lines: count, prefix, emit -- a table of exactly n_lines + 1 entries
    const uint64_t tiles = (n + svx_sam::TILE - 1) / svx_sam::TILE;
    std::vector<uint64_t> tile_base(tiles + 1, 0);
    for (uint64_t b = 0; b < tiles; ++b) {
        uint64_t c = 0;
        for (uint32_t t = 0; t < svx_sam::THREADS; ++t) c += svx_sam::count_newlines(text, n, b, t);
        tile_base[b + 1] = tile_base[b] + c;
    }
    const bool open = n > 0 && text[n - 1] != '\n';
    const uint64_t n_lines = tile_base[tiles] + open, cap = n_lines + 1;
    int64_t* line_off = static_cast<int64_t*>(malloc(cap * sizeof(int64_t)));
    line_off[0] = 0;
    if (open) line_off[n_lines] = (int64_t)n;
    for (uint64_t b = 0; b < tiles; ++b) {
        uint64_t rank = tile_base[b];
        for (uint32_t t = 0; t < svx_sam::THREADS; ++t) {
            svx_sam::emit_newlines(text, n, b, t, rank, line_off, cap);
            rank += svx_sam::count_newlines(text, n, b, t);
        }
    }
    // ---- measure: a wave a line
    Wave w;
    std::vector<int32_t> len(n_lines), tid(n_lines), pos(n_lines), flag(n_lines), span(n_lines);
    for (uint64_t i = 0; i < n_lines; ++i)
        svx_sam::measure_line(w, text, line_off, i, rt, len.data(), tid.data(), pos.data(), flag.data(), span.data());
    // ---- encode: the records end to end in a block of exactly their bytes, at a base the kernel subtracts
    std::vector<int64_t> off(n_lines + 1, 0);
    const int64_t out_base = 1000;
    off[0] = out_base;
    for (uint64_t i = 0; i < n_lines; ++i) off[i + 1] = off[i] + (len[i] > 0 ? len[i] : 0);
    const int64_t total = off[n_lines] - out_base;
    uint8_t* out = static_cast<uint8_t*>(malloc((size_t)(total ? total : 1)));
    memset(out, 0xA5, (size_t)(total ? total : 1));
    int32_t status = 0;
    for (uint64_t i = 0; i < n_lines; ++i)
        svx_sam::encode_line(w, text, line_off, i, rt, len.data(), off.data(), out_base, out, &status);
    // a line that no longer measures its length is refused, and nothing is written: the first record, a byte short
    if (n_lines && len[0] > 0) {
        std::vector<int32_t> wrong(len);
        wrong[0] -= 1;
        int32_t refused = 0;
        uint8_t* one = static_cast<uint8_t*>(malloc((size_t)wrong[0] ? (size_t)wrong[0] : 1));
        memset(one, 0xA5, (size_t)wrong[0] ? (size_t)wrong[0] : 1);
        svx_sam::encode_line(w, text, line_off, 0, rt, wrong.data(), off.data(), out_base, one, &refused);
        bool untouched = refused == 1;
        for (int32_t k = 0; k < wrong[0]; ++k) untouched = untouched && one[k] == 0xA5;
        free(one);
        if (!untouched) { fprintf(stderr, "a wrong length was not refused\n"); return 1; }
    }
    FILE* f = fopen(argv[3], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    const int64_t n64 = (int64_t)n_lines;
    put(f, &n64, 1);
    put(f, line_off, (size_t)cap);
    put(f, len.data(), len.size()); put(f, tid.data(), tid.size()); put(f, pos.data(), pos.size()); put(f, flag.data(), flag.size());
    put(f, span.data(), span.size());
    put(f, &status, 1);
    put(f, &total, 1);
    put(f, out, (size_t)total);
    fclose(f);
    free(out); free(line_off); free(text);
    printf("%llu lines, %lld record bytes, status %d\n", (unsigned long long)n_lines, (long long)total, status);
    return 0;
}
