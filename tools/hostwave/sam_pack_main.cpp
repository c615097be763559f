// The SAM pack kernels (svx_sam_pack_count / svx_sam_pack_extract, svision_amd/csrc/svx_sam.hip) without a GPU: the phases of
// svx_sam_core.hpp -- the code the kernels run -- as loops over lanes and lines.  Built with -fsanitize=address,undefined: the text lies
// in a heap block of exactly its bytes + the 64 bytes of slack include/svx.h asks for, every output array in one of exactly its size;
// every read or write outside is reported.
// Build: g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// usage: sam_pack_host TEXT NAMES OUT WITH_SEQ   TEXT: alignment lines; NAMES: the reference names in tid order, a line each; WITH_SEQ: 0
//                                  or 1.  OUT receives, little endian: int64 n_lines, int32 status [n], int32 fields [5][n] (tid pos
//                                  flag mapq l_seq), int32 counts [3][n] (words, name bytes, SEQ bytes), what the extract wrote -- int32
//                                  tid pos l_seq [n] each, int16 flag [n], uint8 mapq [n] (0xA5 bytes where a line is not taken) --,
//                                  int64 the totals of the three counts, the words, the name bytes, the SEQ bytes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../svision_amd/csrc/svx_sam_core.hpp"

// the wave as the phases see it: its lanes one after the other
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

// a heap block of exactly n elements (one byte where n is 0: nothing is written there), every byte 0xA5
template <class T> static T* exactly(size_t n)
{
    const size_t bytes = n * sizeof(T) ? n * sizeof(T) : 1;
    T* p = static_cast<T*>(malloc(bytes));
    memset(p, 0xA5, bytes);
    return p;
}

int main(int argc, char** argv)
{
    if (argc != 5) { fprintf(stderr, "usage: sam_pack_host TEXT NAMES OUT WITH_SEQ\n"); return 2; }
    const std::vector<uint8_t> file = slurp(argv[1]), names_file = slurp(argv[2]);
    const bool with_seq = atoi(argv[4]) != 0;
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
    // ---- the line table (the line kernels have sam_main.cpp for their model: here the newlines are simply found)
    std::vector<int64_t> starts(1, 0);
    for (uint64_t p = 0; p < n; ++p) if (text[p] == '\n') starts.push_back((int64_t)p + 1);
    if (n > 0 && text[n - 1] != '\n') starts.push_back((int64_t)n);
    const uint64_t n_lines = starts.size() - 1;
    int64_t* line_off = exactly<int64_t>(n_lines + 1);
    memcpy(line_off, starts.data(), (n_lines + 1) * sizeof(int64_t));
    // ---- count: a wave a line
    Wave w;
    int32_t* status = exactly<int32_t>(n_lines);
    int32_t* fields = exactly<int32_t>(5 * n_lines);
    int32_t* counts = exactly<int32_t>(3 * n_lines);
    for (uint64_t i = 0; i < n_lines; ++i) svx_sam::pack_count_line(w, text, line_off, i, n_lines, rt, with_seq, status, fields, counts);
    // ---- the caller's prefix over the counts (a line that is not taken has none), arrays of exactly the totals
    int64_t* off[3];
    for (int k = 0; k < 3; ++k) {
        off[k] = exactly<int64_t>(n_lines + 1);
        off[k][0] = 0;
        for (uint64_t i = 0; i < n_lines; ++i) off[k][i + 1] = off[k][i] + (status[i] == 0 ? counts[k * n_lines + i] : 0);
    }
    const int64_t totals[3] = {off[0][n_lines], off[1][n_lines], off[2][n_lines]};
    int32_t* tid = exactly<int32_t>(n_lines);
    int32_t* pos = exactly<int32_t>(n_lines);
    int32_t* l_seq = exactly<int32_t>(n_lines);
    int16_t* flag = exactly<int16_t>(n_lines);
    uint8_t* mapq = exactly<uint8_t>(n_lines);
    uint32_t* cigar = exactly<uint32_t>((size_t)totals[0]);
    uint8_t* name_bytes = exactly<uint8_t>((size_t)totals[1]);
    uint8_t* seq = exactly<uint8_t>((size_t)totals[2]);
    const svx_sam::PackOut out{tid, pos, l_seq, flag, mapq, off[0], cigar, off[1], name_bytes, with_seq ? off[2] : nullptr, with_seq ? seq : nullptr};
    for (uint64_t i = 0; i < n_lines; ++i) svx_sam::pack_extract_line(w, text, line_off, i, rt, status, out);
    // offsets that are not the counts' prefix write nowhere: the first taken line again, every slot a unit short, into blocks of those sizes
    for (uint64_t i = 0; i < n_lines; ++i) {
        if (status[i] != 0 || counts[i] < 1) continue;
        const int64_t c = counts[i] - 1, nb = counts[n_lines + i] - 1, sb = counts[2 * n_lines + i] > 0 ? counts[2 * n_lines + i] - 1 : 0;
        std::vector<int64_t> o0(n_lines + 1, 0), o1(n_lines + 1, 0), o2(n_lines + 1, 0);
        for (uint64_t k = i + 1; k <= n_lines; ++k) { o0[k] = c; o1[k] = nb; o2[k] = sb; }
        uint32_t* c2 = exactly<uint32_t>((size_t)c);
        uint8_t* n2 = exactly<uint8_t>((size_t)nb);
        uint8_t* s2 = exactly<uint8_t>((size_t)sb);
        const svx_sam::PackOut shorter{tid, pos, l_seq, flag, mapq, o0.data(), c2, o1.data(), n2, with_seq ? o2.data() : nullptr, with_seq ? s2 : nullptr};
        svx_sam::pack_extract_line(w, text, line_off, i, rt, status, shorter);
        bool untouched = true;
        for (int64_t k = 0; k < nb; ++k) untouched = untouched && n2[k] == 0xA5;
        for (int64_t k = 0; k < sb; ++k) untouched = untouched && s2[k] == 0xA5;
        free(c2); free(n2); free(s2);
        if (!untouched) { fprintf(stderr, "a slot of another size was written\n"); return 1; }
        break;
    }
    FILE* f = fopen(argv[3], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    const int64_t n64 = (int64_t)n_lines;
    put(f, &n64, 1);
    put(f, status, n_lines); put(f, fields, 5 * n_lines); put(f, counts, 3 * n_lines);
    put(f, tid, n_lines); put(f, pos, n_lines); put(f, l_seq, n_lines); put(f, flag, n_lines); put(f, mapq, n_lines);
    put(f, totals, 3);
    put(f, cigar, (size_t)totals[0]); put(f, name_bytes, (size_t)totals[1]); put(f, seq, (size_t)totals[2]);
    fclose(f);
    for (int k = 0; k < 3; ++k) free(off[k]);
    free(tid); free(pos); free(l_seq); free(flag); free(mapq); free(cigar); free(name_bytes); free(seq);
    free(status); free(fields); free(counts); free(line_off); free(text);
    printf("%llu lines, %lld words, %lld name bytes, %lld SEQ bytes\n", (unsigned long long)n_lines, (long long)totals[0], (long long)totals[1],
           (long long)totals[2]);
    return 0;
}
