// record_tags_measure_kernel and record_tags_write_kernel (svision_amd/csrc/svx_recsort.hip) without a GPU: the wave routines of
// svx_recsort_core.hpp -- the code the kernels run -- as a loop over the 64 lanes of every record's wave, a ballot as a loop over the
// lanes.  Built with -fsanitize=address,undefined.  measure runs on the record bytes in a heap block of EXACTLY their size: it reads
// byte by byte, and any read outside is reported.  write runs on a copy that is readable up to the next multiple of 4 and not a byte
// more (the slack include/svx.h states: the copy routine reads aligned dwords) and writes into a heap block of exactly the new
// records' bytes; every write outside is reported.  The table is a heap block of exactly SVX_RECORD_TAGS_TABLE_BYTES bytes.
// Build: g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// usage: tags_host IN OUT
//   IN   int64 n, n_bytes; int64 off[n + 1]; uint8 table[8192]; uint8 bytes[n_bytes]
//   OUT  int32 status of measure, of write; int64 new_len[n]; int64 n_out; uint8 out[n_out]     -- measure, an exclusive sum, write
// The caller (tests/tagcases.py) crafts the stream and compares every byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../svision_amd/csrc/svx_recsort_core.hpp"

template <class T>
static T* read_exact(FILE* f, size_t count)
{
    T* p = static_cast<T*>(malloc(count * sizeof(T)));          // (count 0: a block of no byte, any access is reported)
    if (count && fread(p, sizeof(T), count, f) != count) { fprintf(stderr, "tags_host: the input is cut\n"); exit(2); }
    return p;
}

// A copy of p[0 .. count) that is 4-byte aligned and readable up to the next multiple of 4.
static uint8_t* padded_copy(const uint8_t* p, size_t count)
{
    const size_t size = (count + 3) / 4 * 4;
    uint8_t* q = static_cast<uint8_t*>(aligned_alloc(4, size ? size : 4));
    memset(q, 0xEE, size ? size : 4);
    if (count) memcpy(q, p, count);
    return q;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: tags_host IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t* head = read_exact<int64_t>(f, 2);
    const int64_t n = head[0], n_bytes = head[1];
    if (n < 0 || n > 0xFFFFFFFFll || n_bytes < 0) { fprintf(stderr, "tags_host: a bad head\n"); return 2; }
    int64_t* off = read_exact<int64_t>(f, (size_t)n + 1);
    uint32_t* table = read_exact<uint32_t>(f, svx_recsort::TAGS_TABLE_WORDS);
    uint8_t* bytes = read_exact<uint8_t>(f, (size_t)n_bytes);
    fclose(f);
    for (int64_t r = 0; r <= n; ++r)
        if (off[r] < 0 || off[r] > n_bytes || (r && off[r] < off[r - 1])) { fprintf(stderr, "tags_host: record %lld does not lie in the bytes\n", (long long)r); return 2; }

    int32_t status[2] = {0, 0};
    int64_t* new_len = static_cast<int64_t*>(malloc((size_t)n * sizeof(int64_t)));
    int64_t* new_off = static_cast<int64_t*>(malloc(((size_t)n + 1) * sizeof(int64_t)));
    for (uint64_t r = 0; r < (uint64_t)n; ++r)                   // the measure kernel's waves, lane by lane
        for (uint32_t lane = 0; lane < svx_recsort::WAVE; ++lane)
            svx_recsort::tags_measure_record(bytes, off, table, new_len, r, lane, &status[0]);
    new_off[0] = 0;
    for (int64_t r = 0; r < n; ++r) new_off[r + 1] = new_off[r] + new_len[r];
    const int64_t n_out = new_off[n];

    uint8_t* bytes4 = padded_copy(bytes, (size_t)n_bytes);
    uint8_t* out = static_cast<uint8_t*>(malloc((size_t)n_out));
    if (n_out) memset(out, 0xA5, (size_t)n_out);
    for (uint64_t r = 0; r < (uint64_t)n; ++r)                   // the write kernel's waves
        for (uint32_t lane = 0; lane < svx_recsort::WAVE; ++lane)
            svx_recsort::tags_write_record(bytes4, off, table, new_off, out, r, lane, &status[1]);

    FILE* g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    fwrite(status, sizeof(int32_t), 2, g);
    if (n) fwrite(new_len, sizeof(int64_t), (size_t)n, g);
    fwrite(&n_out, sizeof n_out, 1, g);
    if (n_out) fwrite(out, 1, (size_t)n_out, g);
    fclose(g);
    printf("%lld records, %lld -> %lld bytes, status %d %d\n", (long long)n, (long long)(n ? off[n] - off[0] : 0), (long long)n_out, status[0], status[1]);
    free(head); free(off); free(table); free(bytes); free(new_len); free(new_off); free(bytes4); free(out);
    return 0;
}
