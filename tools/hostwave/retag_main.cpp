// record_retag_measure_kernel and record_retag_write_kernel (svision_amd/csrc/svx_recsort.hip) without a GPU: the wave routines of
// svx_recsort_core.hpp -- the code the kernels run -- as a loop over the 64 lanes of every record's wave, a ballot as a loop over the
// lanes.  Built with -fsanitize=address,undefined.  measure runs on the record bytes in a heap block of EXACTLY their size and on a
// table of exactly its size: it reads byte by byte, and any read outside is reported.  write runs on copies that are readable up to
// the next multiple of 4 (what include/svx.h asks for: the copy routine reads aligned dwords) and writes into a heap block of
// exactly the new records' bytes; every write outside is reported.
// Build: g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// usage: retag_host IN OUT
//   IN   int64 n, m, n_bytes, n_table; int64 off[n + 1]; int32 table_off[2m + 1]; uint8 table[n_table]; uint8 bytes[n_bytes]
//   OUT  int32 status of measure, of write; int64 new_len[n]; int64 n_out; uint8 out[n_out]     -- measure, an exclusive sum, write
// The caller (tests/retagcases.py) crafts the stream and compares every byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../svision_amd/csrc/svx_recsort_core.hpp"

template <class T>
static T* read_exact(FILE* f, size_t count)
{
    T* p = static_cast<T*>(malloc(count * sizeof(T)));          // (count 0: a block of no byte, any access is reported)
    if (count && fread(p, sizeof(T), count, f) != count) { fprintf(stderr, "retag_host: the input is cut\n"); exit(2); }
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
    if (argc != 3) { fprintf(stderr, "usage: retag_host IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t* head = read_exact<int64_t>(f, 4);
    const int64_t n = head[0], m = head[1], n_bytes = head[2], n_table = head[3];
    if (n < 0 || n > 0xFFFFFFFFll || m < 0 || m > 0x3FFFFFFF || n_bytes < 0 || n_table < 0) { fprintf(stderr, "retag_host: a bad head\n"); return 2; }
    int64_t* off = read_exact<int64_t>(f, (size_t)n + 1);
    int32_t* table_off = read_exact<int32_t>(f, (size_t)(2 * m + 1));
    uint8_t* table = read_exact<uint8_t>(f, (size_t)n_table);
    uint8_t* bytes = read_exact<uint8_t>(f, (size_t)n_bytes);
    fclose(f);
    for (int64_t r = 0; r <= n; ++r)
        if (off[r] < 0 || off[r] > n_bytes || (r && off[r] < off[r - 1])) { fprintf(stderr, "retag_host: record %lld does not lie in the bytes\n", (long long)r); return 2; }
    for (int64_t e = 0; e <= 2 * m; ++e)
        if (table_off[e] < 0 || table_off[e] > n_table || (e && table_off[e] < table_off[e - 1] + (e % 2 ? 2 : 0))) { fprintf(stderr, "retag_host: a bad table\n"); return 2; }

    int32_t status[2] = {0, 0};
    int64_t* new_len = static_cast<int64_t*>(malloc((size_t)n * sizeof(int64_t)));
    int64_t* new_off = static_cast<int64_t*>(malloc(((size_t)n + 1) * sizeof(int64_t)));
    const svx_recsort::RetagTable exact{table, table_off, (int32_t)m};
    for (uint64_t r = 0; r < (uint64_t)n && m; ++r)              // the measure kernel's waves, lane by lane
        for (uint32_t lane = 0; lane < svx_recsort::WAVE; ++lane)
            svx_recsort::retag_measure_record(bytes, off, exact, new_len, r, lane, &status[0]);
    for (int64_t r = 0; r < n && !m; ++r) new_len[r] = off[r + 1] - off[r];         // (an empty table launches nothing)
    new_off[0] = 0;
    for (int64_t r = 0; r < n; ++r) new_off[r + 1] = new_off[r] + new_len[r];
    const int64_t n_out = new_off[n];

    uint8_t* bytes4 = padded_copy(bytes, (size_t)n_bytes);
    uint8_t* table4 = padded_copy(table, (size_t)n_table);
    const svx_recsort::RetagTable padded{table4, table_off, (int32_t)m};
    uint8_t* out = static_cast<uint8_t*>(malloc((size_t)n_out));
    if (n_out) memset(out, 0xA5, (size_t)n_out);
    for (uint64_t r = 0; r < (uint64_t)n && m; ++r)              // the write kernel's waves
        for (uint32_t lane = 0; lane < svx_recsort::WAVE; ++lane)
            svx_recsort::retag_write_record(bytes4, off, padded, new_off, out, r, lane, &status[1]);
    if (!m && n_out) memcpy(out, bytes + off[0], (size_t)n_out);

    FILE* g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    fwrite(status, sizeof(int32_t), 2, g);
    if (n) fwrite(new_len, sizeof(int64_t), (size_t)n, g);
    fwrite(&n_out, sizeof n_out, 1, g);
    if (n_out) fwrite(out, 1, (size_t)n_out, g);
    fclose(g);
    printf("%lld records, %lld -> %lld bytes, status %d %d\n", (long long)n, (long long)(n ? off[n] - off[0] : 0), (long long)n_out, status[0], status[1]);
    free(head); free(off); free(table_off); free(table); free(bytes); free(new_len); free(new_off); free(bytes4); free(table4); free(out);
    return 0;
}
