// record_retid_kernel (svision_amd/csrc/svx_recsort.hip) without a GPU: the lane routine of svx_recsort_core.hpp -- the code the
// kernel runs -- as a loop over the records.  Built with -fsanitize=address,undefined: the record bytes lie in a heap block of exactly
// their size, offsets, table and keys in blocks of exactly theirs; every read or write outside is reported.
// Build: g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// usage: retid_host IN OUT
//   IN   int64 n, n_in, n_bytes, has_key; int64 off[n]; int32 map[n_in]; int32 key[n] (has_key); uint8 bytes[n_bytes]
//   OUT  int32 status; int32 key[n] (has_key); uint8 bytes[n_bytes]      -- what the launch leaves
// The caller (tests/test_sort_merge_cpu.py) crafts the stream with its sentinels and compares every byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../svision_amd/csrc/svx_recsort_core.hpp"

template <class T>
static T* read_exact(FILE* f, size_t count)
{
    T* p = static_cast<T*>(malloc(count * sizeof(T)));          // (count 0: a block of no byte, any access is reported)
    if (count && fread(p, sizeof(T), count, f) != count) { fprintf(stderr, "retid_host: the input is cut\n"); exit(2); }
    return p;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: retid_host IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t* head = read_exact<int64_t>(f, 4);
    const int64_t n = head[0], n_in = head[1], n_bytes = head[2], has_key = head[3];
    if (n < 0 || n > 0xFFFFFFFFll || n_in < 0 || n_in > 0x7FFFFFFF || n_bytes < 0) { fprintf(stderr, "retid_host: a bad head\n"); return 2; }
    int64_t* off = read_exact<int64_t>(f, (size_t)n);
    int32_t* map = read_exact<int32_t>(f, (size_t)n_in);
    int32_t* key = has_key ? read_exact<int32_t>(f, (size_t)n) : nullptr;
    uint8_t* bytes = read_exact<uint8_t>(f, (size_t)n_bytes);
    fclose(f);
    for (int64_t r = 0; r < n; ++r)
        if (off[r] < 0 || off[r] + 28 > n_bytes) { fprintf(stderr, "retid_host: record %lld does not lie in the bytes\n", (long long)r); return 2; }
    int32_t status = 0;
    for (uint64_t r = 0; r < (uint64_t)n; ++r)                   // the kernel's lanes, one record each
        svx_recsort::retid_record(bytes, off, map, (int32_t)n_in, key, r, &status);
    FILE* g = fopen(argv[2], "wb");
    if (!g) { perror(argv[2]); return 2; }
    fwrite(&status, sizeof status, 1, g);
    if (key && n) fwrite(key, sizeof(int32_t), (size_t)n, g);
    if (n_bytes) fwrite(bytes, 1, (size_t)n_bytes, g);
    fclose(g);
    printf("%lld records, status %d\n", (long long)n, status);
    free(head); free(off); free(map); free(key); free(bytes);
    return 0;
}
