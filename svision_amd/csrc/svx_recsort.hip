// svx_recsort.hip -- the records of an unsorted BAM in coordinate order, on the device (gfx950).
//
// The record walk (svx_bamdev.hip) takes a BAM apart in FILE order; everything behind it -- the CIGAR scan's windows, the
// collection -- wants the order of `samtools sort`: by (reference, position), records without a reference last, equal keys
// in file order.  svx_record_sort gives the permutation, the gathers apply it to the walk's arrays.
//
//   svx_record_sort   a stable LSD radix sort, 8 bits a pass, over the SIGNIFICANT bits only: the key
//                     ((tid < 0 ? n_ref : tid) << pos_bits) | (pos + 1) has pos_bits + bit_length(n_ref) of them (human
//                     genome, 3,366 references: 28 + 12 = 5 passes, not 8).  (key, index) pairs travel between two buffers.
//     hist            a workgroup per tile of SVX_RECORD_SORT_TILE elements -> table[digit][tile] = how many of the tile's
//                     elements have that digit
//     scan            ONE exclusive prefix sum over the whole 256 x tiles table, digit-major: entry [d][t] becomes the first
//                     output position of tile t's elements with digit d (chunk sums, one workgroup over the sums, chunks again)
//     scatter         the tile again.  Element e of a tile belongs to wave e / 512, round (e / 64) % 8, lane e % 64 -- waves,
//                     rounds and lanes taken in that order ARE the input order.  A round: eight ballots give every lane the
//                     mask of the lanes of its wave that hold the same digit; the lanes below it in that mask are its rank in the
//                     round, the lowest lane of the mask (the leader) keeps the wave's running count of the digit in LDS.  Then
//                     thread d turns the four waves' counts of digit d into their first positions, and every element goes to
//                     table[d][tile] + (its digit in earlier waves) + (in earlier rounds of its wave) + (in lower lanes).
//   svx_record_gather           dst[r] = src[order[r]], elements of 1, 2 or 4 bytes (tid, pos, flag, mapq, l_seq)
//   svx_record_gather_offsets   off_out[r] = sum of the lengths of the segments order[0 .. r), the same three-launch scan (int64)
//   svx_record_gather_segments  a WAVE per record copies segment order[r] to off_out[r]: aligned dword stores, the source read in
//                               aligned dwords and shifted into place, at most 3 single bytes at either end
//   svx_record_invert           rank[order[r]] = r: the sorted rank of every input record
//   svx_record_scatter_segments the gather turned round, for a record stream that is taken in pieces (svision_amd/sort.py, a file
//                               larger than the device): a WAVE per INPUT record; where the record's rank lies in the window
//                               [rank_lo, rank_hi) its bytes go to off_out[rank] - out_base, by the copy routine of
//                               svx_recsort_core.hpp (the gather's alignment rule); the other waves leave at once
//   svx_record_retid            a LANE per record rewrites its refID and next_refID through a table (several inputs merged into one
//                               file, svision_amd/sort.py: each input's indices into the merged dictionary), byte by byte in place
//   svx_record_retag_measure    a WAVE per record walks the optional fields behind qual and finds the first RG:Z / PG:Z value that a
//   svx_record_retag_write      table renames (the IDs of several inputs that collide, svision_amd/sort.py): the new length, then the
//                               record with the value replaced and block_size set, in up to five copies (svx_recsort_core.hpp)
//   svx_record_tags_measure     a WAVE per record walks the same chain and removes optional fields by their tag (svision_amd/sort.py,
//   svx_record_tags_write       --drop-tags / --keep-tags): one bit a two-byte tag in a bitmap of 65,536; the new length, then the
//                               record without them, a copy a run of kept fields, block_size set (svx_recsort_core.hpp)
// No atomics, no cross-workgroup dependency inside a launch: the output is a pure function of the input, identical in every run.
// A counter in LDS is written by ONE lane a round (the leader of its digit, in the wave's own row) with a barrier behind it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/svx.h"
#include "svx_recsort_core.hpp"

namespace {

constexpr int WAVE = 64;
constexpr int SORT_BLOCK = 256, SORT_WAVES = SORT_BLOCK / WAVE, SORT_ROUNDS = 8, RADIX = 256;
constexpr uint32_t SORT_TILE = SORT_BLOCK * SORT_ROUNDS;
static_assert(SORT_TILE == SVX_RECORD_SORT_TILE, "include/svx.h names the tile");
static_assert(SORT_BLOCK == RADIX, "thread d sums digit d");
constexpr int SCAN_BLOCK = 256, SCAN_ITEMS = 4, SCAN_WAVES = SCAN_BLOCK / WAVE;
constexpr uint32_t SCAN_CHUNK = SCAN_BLOCK * SCAN_ITEMS;         // values a workgroup of the scan takes
constexpr int SEG_WAVES = 4;                                    // gather_segments: four records a workgroup, a wave each
constexpr uint64_t RETID_MAX_BLOCKS = 2048;                     // record_retid: workgroups of 256 lanes (256 CUs x 8); more records: the grid-stride loop

__host__ __device__ inline uint64_t pad16(uint64_t v) { return (v + 15) / 16 * 16; }

__host__ __device__ inline uint32_t bit_length(uint32_t v)
{
    uint32_t b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

struct Key {                                                    // what makes a record's key (the head of the file)
    uint32_t n_ref, pos_bits;
};

__device__ __forceinline__ uint64_t key_of(int32_t tid, int32_t pos, Key k)
{
    const uint64_t hi = (uint32_t)tid >= k.n_ref ? k.n_ref : (uint32_t)tid;      // (tid < 0, and what no dictionary names: last)
    const uint32_t lo = (uint32_t)pos + 1u;
    return hi << k.pos_bits | (k.pos_bits >= 32 ? lo : lo & ((1u << k.pos_bits) - 1u));
}

// Element i of a pass's input: the first pass makes the keys (index = i), the later ones read what the pass before wrote.
template <bool FIRST>
__device__ __forceinline__ void load_element(uint64_t i, const int32_t* __restrict__ tid, const int32_t* __restrict__ pos, Key k,
                                             const uint64_t* __restrict__ key_in, const uint32_t* __restrict__ idx_in, uint64_t* key, uint32_t* idx)
{
    if (FIRST) {
        *key = key_of(tid[i], pos[i], k);
        *idx = (uint32_t)i;
    } else {
        *key = key_in[i];
        *idx = idx_in[i];
    }
}

// The lanes of the wave that are `valid` and hold digit d (every lane of the wave calls this: eight ballots).
__device__ __forceinline__ uint64_t same_digit(uint32_t d, bool valid)
{
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool set = (d >> b) & 1u;
        const uint64_t with = __ballot(valid && set);
        peers &= set ? with : ~with;
    }
    return peers;
}

template <bool FIRST>
__global__ __launch_bounds__(SORT_BLOCK)
void sort_hist_kernel(const int32_t* __restrict__ tid, const int32_t* __restrict__ pos, Key k, const uint64_t* __restrict__ key_in,
                      const uint32_t* __restrict__ idx_in, uint32_t n, uint32_t shift, uint32_t tiles, uint32_t* __restrict__ table)
{
    __shared__ uint32_t cnt[SORT_WAVES][RADIX];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) cnt[w][t] = 0;
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * SORT_TILE + (uint64_t)wv * (SORT_ROUNDS * WAVE) + lane;
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const uint64_t i = first + (uint64_t)r * WAVE;
        const bool valid = i < n;
        uint64_t key = 0;
        uint32_t idx = 0;
        if (valid) load_element<FIRST>(i, tid, pos, k, key_in, idx_in, &key, &idx);
        const uint32_t d = (uint32_t)(key >> shift) & 255u;
        const uint64_t peers = same_digit(d, valid);
        if (valid && lane == (uint32_t)__ffsll((unsigned long long)peers) - 1u) cnt[wv][d] += (uint32_t)__popcll(peers);
        __syncthreads();                                        // the next round's leader of this digit may be another lane
    }
    table[(uint64_t)t * tiles + blockIdx.x] = cnt[0][t] + cnt[1][t] + cnt[2][t] + cnt[3][t];
}

template <bool FIRST>
__global__ __launch_bounds__(SORT_BLOCK)
void sort_scatter_kernel(const int32_t* __restrict__ tid, const int32_t* __restrict__ pos, Key k, const uint64_t* __restrict__ key_in,
                         const uint32_t* __restrict__ idx_in, uint32_t n, uint32_t shift, uint32_t tiles, const uint32_t* __restrict__ table,
                         uint64_t* __restrict__ key_out, uint32_t* __restrict__ idx_out)
{
    __shared__ uint32_t cnt[SORT_WAVES][RADIX];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) cnt[w][t] = 0;
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * SORT_TILE + (uint64_t)wv * (SORT_ROUNDS * WAVE) + lane;
    uint64_t key[SORT_ROUNDS];
    uint32_t idx[SORT_ROUNDS], rank[SORT_ROUNDS];
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        const uint64_t i = first + (uint64_t)r * WAVE;
        const bool valid = i < n;
        key[r] = 0;
        idx[r] = 0;
        if (valid) load_element<FIRST>(i, tid, pos, k, key_in, idx_in, &key[r], &idx[r]);
        const uint32_t d = (uint32_t)(key[r] >> shift) & 255u;
        const uint64_t peers = same_digit(d, valid);
        const uint32_t leader = valid ? (uint32_t)__ffsll((unsigned long long)peers) - 1u : lane;
        uint32_t before = 0;                                    // the digit's count in the wave's earlier rounds: the leader reads and adds
        if (valid && lane == leader) {
            before = cnt[wv][d];
            cnt[wv][d] = before + (uint32_t)__popcll(peers);
        }
        before = __shfl(before, (int)leader);
        rank[r] = before + (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        __syncthreads();
    }
    // thread d: where each wave's elements with digit d begin -- the tile's first position of d, then the waves in order
    uint32_t run = table[(uint64_t)t * tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) {
        const uint32_t c = cnt[w][t];
        cnt[w][t] = run;
        run += c;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_ROUNDS; ++r) {
        if (first + (uint64_t)r * WAVE < n) {
            const uint32_t at = cnt[wv][(uint32_t)(key[r] >> shift) & 255u] + rank[r];
            if (key_out) key_out[at] = key[r];
            idx_out[at] = idx[r];
        }
    }
}

// ---- exclusive prefix sum over any number of values, three launches ----
// The scanned sequence: the sort's table as it stands, or the lengths of the segments in their new order.
struct TableValues {
    const uint32_t* v;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return v[i]; }
};
struct SegmentLengths {
    const int64_t* off;
    const uint32_t* order;
    __device__ __forceinline__ int64_t operator()(uint64_t r) const { const uint32_t s = order[r]; return off[(uint64_t)s + 1] - off[s]; }
};

// Exclusive prefix of `mine` over the workgroup's threads in order, *total = the sum over all of them (two barriers).
template <typename T>
__device__ __forceinline__ T block_exclusive(T mine, T* wave_sum, T* total)
{
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    T inc = mine;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const T v = __shfl_up(inc, o);
        if ((int)lane >= o) inc += v;
    }
    if (lane == 63) wave_sum[wv] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w) {
        const T s = wave_sum[w];
        if (w < (int)wv) before += s;
        all += s;
    }
    __syncthreads();                                            // wave_sum may be written again
    *total = all;
    return before + inc - mine;
}

template <typename T, typename In>
__global__ __launch_bounds__(SCAN_BLOCK)
void scan_sums_kernel(In in, uint64_t count, T* __restrict__ sums)
{
    __shared__ T wave_sum[SCAN_WAVES];
    const uint64_t i0 = (uint64_t)blockIdx.x * SCAN_CHUNK + (uint64_t)threadIdx.x * SCAN_ITEMS;
    T mine = 0;
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e)
        if (i0 + e < count) mine += in(i0 + e);
    T total;
    block_exclusive(mine, wave_sum, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// ONE workgroup: the chunk sums -> their exclusive prefix, SCAN_BLOCK of them a step; *total (if wanted) = the sum of everything.
template <typename T, typename Out>
__global__ __launch_bounds__(SCAN_BLOCK)
void scan_top_kernel(T* __restrict__ sums, uint32_t chunks, Out* __restrict__ total_out)
{
    __shared__ T wave_sum[SCAN_WAVES];
    T carry = 0;
    for (uint32_t c0 = 0; c0 < chunks; c0 += SCAN_BLOCK) {
        const uint32_t c = c0 + threadIdx.x;
        const T mine = c < chunks ? sums[c] : (T)0;
        T total;
        const T ex = block_exclusive(mine, wave_sum, &total);
        if (c < chunks) sums[c] = carry + ex;
        carry += total;
    }
    if (total_out && threadIdx.x == 0) *total_out = (Out)carry;
}

// Every chunk again: its values' exclusive prefix, behind the chunk's own (out may be the array `in` reads: a thread reads its
// values before it writes them, and nobody else's).
template <typename T, typename In, typename Out>
__global__ __launch_bounds__(SCAN_BLOCK)
void scan_apply_kernel(In in, uint64_t count, const T* __restrict__ sums, Out* out)
{
    __shared__ T wave_sum[SCAN_WAVES];
    const uint64_t i0 = (uint64_t)blockIdx.x * SCAN_CHUNK + (uint64_t)threadIdx.x * SCAN_ITEMS;
    T v[SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) {
        v[e] = i0 + e < count ? (T)in(i0 + e) : (T)0;
        mine += v[e];
    }
    T total;
    T at = sums[blockIdx.x] + block_exclusive(mine, wave_sum, &total);
#pragma unroll
    for (int e = 0; e < SCAN_ITEMS; ++e) {
        if (i0 + e < count) out[i0 + e] = (Out)at;
        at += v[e];
    }
}

template <typename T, typename In, typename Out>
void exclusive_scan(In in, uint64_t count, T* sums, Out* out, Out* total_out, hipStream_t st)
{
    const uint32_t chunks = (uint32_t)((count + SCAN_CHUNK - 1) / SCAN_CHUNK);
    hipLaunchKernelGGL((scan_sums_kernel<T, In>), dim3(chunks), dim3(SCAN_BLOCK), 0, st, in, count, sums);
    hipLaunchKernelGGL((scan_top_kernel<T, Out>), dim3(1), dim3(SCAN_BLOCK), 0, st, sums, chunks, total_out);
    hipLaunchKernelGGL((scan_apply_kernel<T, In, Out>), dim3(chunks), dim3(SCAN_BLOCK), 0, st, in, count, sums, out);
}

// ---- the gathers ----
template <typename T>
__global__ __launch_bounds__(256)
void gather_kernel(const T* __restrict__ src, const uint32_t* __restrict__ order, T* __restrict__ dst, uint32_t n)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n) dst[r] = src[order[r]];
}

// A wave per record.  The destination decides the alignment: single bytes up to its first dword boundary, whole dwords -- each
// from the one or two aligned source dwords that hold its bytes --, single bytes behind the last whole dword.
__global__ __launch_bounds__(WAVE * SEG_WAVES)
void gather_segments_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ off_in, const uint32_t* __restrict__ order,
                            const int64_t* __restrict__ off_out, uint8_t* __restrict__ dst, uint32_t n, uint32_t elem_bytes)
{
    const uint64_t r = (uint64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (r >= n) return;                                         // (whole waves: no barrier in this kernel)
    const uint32_t s = order[r];
    const uint64_t len = (uint64_t)(off_in[(uint64_t)s + 1] - off_in[s]) * elem_bytes;
    const uint8_t* from = src + (uint64_t)off_in[s] * elem_bytes;
    uint8_t* to = dst + (uint64_t)off_out[r] * elem_bytes;
    uint64_t head = (uint64_t)(-reinterpret_cast<uintptr_t>(to) & 3u);
    if (head > len) head = len;
    if (lane < head) to[lane] = from[lane];
    const uint64_t words = (len - head) / 4;
    const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(from + head) & 3u), shift = skew * 8;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(from + head - skew);
    uint32_t* out = reinterpret_cast<uint32_t*>(to + head);
    for (uint64_t j = lane; j < words; j += WAVE) {
        uint32_t v = in[j];
        if (shift) v = v >> shift | in[j + 1] << (32 - shift);  // (in[j + 1] holds the word's last byte: inside the segment's dwords)
        out[j] = v;
    }
    const uint64_t done = head + words * 4;
    if (done + lane < len) to[done + lane] = from[done + lane];
}

__global__ __launch_bounds__(256)
void invert_kernel(const uint32_t* __restrict__ order, uint32_t* __restrict__ rank, uint32_t n)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n) rank[order[r]] = (uint32_t)r;
}

// A wave per input record; the destinations of different records are disjoint, a length that does not fit is reported and
// not copied (svx_recsort_core.hpp).
__global__ __launch_bounds__(WAVE * SEG_WAVES)
void scatter_segments_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ src_off, const uint32_t* __restrict__ rank,
                             uint32_t rank_lo, uint32_t rank_hi, const int64_t* __restrict__ off_out, int64_t out_base,
                             uint8_t* __restrict__ dst, uint32_t n, int32_t* __restrict__ status)
{
    const uint64_t i = (uint64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;                                         // (whole waves: no barrier in this kernel)
    svx_recsort::scatter_record(src, src_off, rank, rank_lo, rank_hi, off_out, out_base, dst, i, threadIdx.x & 63u, status);
}

// A lane per record in a grid-stride loop: two fields of four bytes each, at whatever offset the record lies (svx_recsort_core.hpp).
// Two cache lines a record and nothing to share between lanes: the launch is bound by the latency of those loads, not by bandwidth.
__global__ __launch_bounds__(256)
void record_retid_kernel(uint8_t* __restrict__ bytes, const int64_t* __restrict__ off, uint32_t n, const int32_t* __restrict__ map, int32_t n_in,
                         int32_t* __restrict__ tid_key, int32_t* __restrict__ status)
{
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += step)
        svx_recsort::retid_record(bytes, off, map, n_in, tid_key, r, status);
}

// A wave per record (svx_recsort_core.hpp): the field chain is followed by every lane alike, a Z / H value's NUL is found 64 bytes a
// ballot, a B array is skipped from its count.  Long-read records carry arrays of tens of kilobytes; a lane per record would walk
// them alone.
__global__ __launch_bounds__(WAVE * SEG_WAVES)
void record_retag_measure_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off, uint32_t n, svx_recsort::RetagTable table,
                                 int64_t* __restrict__ new_len, int32_t* __restrict__ status)
{
    const uint64_t r = (uint64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;                                         // (whole waves: no barrier in this kernel)
    svx_recsort::retag_measure_record(bytes, off, table, new_len, r, threadIdx.x & 63u, status);
}

__global__ __launch_bounds__(WAVE * SEG_WAVES)
void record_retag_write_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off, uint32_t n, svx_recsort::RetagTable table,
                               const int64_t* __restrict__ new_off, uint8_t* __restrict__ dst, int32_t* __restrict__ status)
{
    const uint64_t r = (uint64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;
    svx_recsort::retag_write_record(bytes, off, table, new_off, dst, r, threadIdx.x & 63u, status);
}

// A wave per record, the retag pair's shape: measure follows the chain and sums the removed fields' bytes, write follows it again and
// copies every run of kept fields by the wave.  Kinetics arrays (fi fp ri rp, B:C of the read's length) are skipped from their count.
__global__ __launch_bounds__(WAVE * SEG_WAVES)
void record_tags_measure_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off, uint32_t n, const uint32_t* __restrict__ table,
                                int64_t* __restrict__ new_len, int32_t* __restrict__ status)
{
    const uint64_t r = (uint64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;                                         // (whole waves: no barrier in this kernel)
    svx_recsort::tags_measure_record(bytes, off, table, new_len, r, threadIdx.x & 63u, status);
}

__global__ __launch_bounds__(WAVE * SEG_WAVES)
void record_tags_write_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off, uint32_t n, const uint32_t* __restrict__ table,
                              const int64_t* __restrict__ new_off, uint8_t* __restrict__ dst, int32_t* __restrict__ status)
{
    const uint64_t r = (uint64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
    if (r >= n) return;
    svx_recsort::tags_write_record(bytes, off, table, new_off, dst, r, threadIdx.x & 63u, status);
}

struct SortWs {
    uint64_t* key[2];
    uint32_t* idx;
    uint32_t* table;
    uint32_t* sums;
};

inline uint32_t sort_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + SORT_TILE - 1) / SORT_TILE); }
inline uint64_t scan_chunks(uint64_t count) { return (count + SCAN_CHUNK - 1) / SCAN_CHUNK; }

}  // namespace

extern "C" size_t svx_record_sort_ws_bytes(uint32_t n)
{
    const uint64_t entries = (uint64_t)RADIX * sort_tiles(n);
    return (size_t)(2 * pad16(8ull * n) + pad16(4ull * n) + pad16(4 * entries) + pad16(4 * scan_chunks(entries)) + 16);
}

extern "C" int svx_record_sort(const int32_t* d_tid, const int32_t* d_pos, uint32_t n, uint32_t n_ref, uint32_t pos_bits,
                               uint32_t* d_order, void* d_ws, uint64_t ws_bytes, void* stream)
{
    if (n == 0) return SVX_OK;
    if (!d_tid || !d_pos || !d_order || !d_ws || pos_bits < 1 || pos_bits > 32 || n_ref > 0x7FFFFFFFu) return SVX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_ws) & 15u) || ws_bytes < svx_record_sort_ws_bytes(n)) return SVX_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t tiles = sort_tiles(n);
    const uint64_t entries = (uint64_t)RADIX * tiles;
    uint8_t* p = static_cast<uint8_t*>(d_ws);
    SortWs w;
    w.key[0] = reinterpret_cast<uint64_t*>(p); p += pad16(8ull * n);
    w.key[1] = reinterpret_cast<uint64_t*>(p); p += pad16(8ull * n);
    w.idx = reinterpret_cast<uint32_t*>(p);    p += pad16(4ull * n);
    w.table = reinterpret_cast<uint32_t*>(p);  p += pad16(4 * entries);
    w.sums = reinterpret_cast<uint32_t*>(p);
    const Key k{n_ref, pos_bits};
    const uint32_t bits = pos_bits + bit_length(n_ref);
    const uint32_t passes = bits ? (bits + 7) / 8 : 1;
    for (uint32_t pass = 0; pass < passes; ++pass) {
        // the index arrays alternate so that the LAST pass writes d_order; the keys alternate too, and the last pass writes none
        const bool last = pass + 1 == passes;
        uint32_t* idx_out = (passes - 1 - pass) % 2 == 0 ? d_order : w.idx;
        const uint32_t* idx_in = idx_out == d_order ? w.idx : d_order;
        uint64_t* key_out = last ? nullptr : w.key[pass % 2];
        const uint64_t* key_in = w.key[(pass + 1) % 2];
        const uint32_t shift = 8 * pass;
        if (pass == 0) {
            hipLaunchKernelGGL(sort_hist_kernel<true>, dim3(tiles), dim3(SORT_BLOCK), 0, st, d_tid, d_pos, k, key_in, idx_in, n, shift, tiles, w.table);
        } else {
            hipLaunchKernelGGL(sort_hist_kernel<false>, dim3(tiles), dim3(SORT_BLOCK), 0, st, d_tid, d_pos, k, key_in, idx_in, n, shift, tiles, w.table);
        }
        exclusive_scan<uint32_t, TableValues, uint32_t>(TableValues{w.table}, entries, w.sums, w.table, nullptr, st);
        if (pass == 0) {
            hipLaunchKernelGGL(sort_scatter_kernel<true>, dim3(tiles), dim3(SORT_BLOCK), 0, st, d_tid, d_pos, k, key_in, idx_in, n, shift, tiles,
                               w.table, key_out, idx_out);
        } else {
            hipLaunchKernelGGL(sort_scatter_kernel<false>, dim3(tiles), dim3(SORT_BLOCK), 0, st, d_tid, d_pos, k, key_in, idx_in, n, shift, tiles,
                               w.table, key_out, idx_out);
        }
    }
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

extern "C" int svx_record_gather(const void* d_src, const uint32_t* d_order, void* d_dst, uint32_t n, uint32_t elem_bytes, void* stream)
{
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return SVX_EINVAL;
    if (n == 0) return SVX_OK;
    if (!d_src || !d_order || !d_dst) return SVX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & (elem_bytes - 1)) return SVX_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((uint32_t)(((uint64_t)n + 255) / 256));
    if (elem_bytes == 1)
        hipLaunchKernelGGL(gather_kernel<uint8_t>, grid, dim3(256), 0, st, static_cast<const uint8_t*>(d_src), d_order, static_cast<uint8_t*>(d_dst), n);
    else if (elem_bytes == 2)
        hipLaunchKernelGGL(gather_kernel<uint16_t>, grid, dim3(256), 0, st, static_cast<const uint16_t*>(d_src), d_order, static_cast<uint16_t*>(d_dst), n);
    else
        hipLaunchKernelGGL(gather_kernel<uint32_t>, grid, dim3(256), 0, st, static_cast<const uint32_t*>(d_src), d_order, static_cast<uint32_t*>(d_dst), n);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

extern "C" size_t svx_record_gather_offsets_ws_bytes(uint32_t n)
{
    return (size_t)(pad16(8 * scan_chunks(n)) + 16);
}

extern "C" int svx_record_gather_offsets(const int64_t* d_off_in, const uint32_t* d_order, uint32_t n, int64_t* d_off_out, void* d_ws,
                                         uint64_t ws_bytes, void* stream)
{
    if (!d_off_out) return SVX_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return hipMemsetAsync(d_off_out, 0, sizeof(int64_t), st) == hipSuccess ? SVX_OK : SVX_ELAUNCH;
    if (!d_off_in || !d_order || !d_ws) return SVX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_ws) & 15u) || ws_bytes < svx_record_gather_offsets_ws_bytes(n)) return SVX_EINVAL;
    exclusive_scan<int64_t, SegmentLengths, int64_t>(SegmentLengths{d_off_in, d_order}, n, static_cast<int64_t*>(d_ws), d_off_out, d_off_out + n, st);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

extern "C" int svx_record_gather_segments(const void* d_src, const int64_t* d_off_in, const uint32_t* d_order, const int64_t* d_off_out,
                                          void* d_dst, uint32_t n, uint32_t elem_bytes, void* stream)
{
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return SVX_EINVAL;
    if (n == 0) return SVX_OK;
    if (!d_src || !d_off_in || !d_order || !d_off_out || !d_dst) return SVX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_src) & 3u) || (reinterpret_cast<uintptr_t>(d_dst) & (elem_bytes - 1))) return SVX_EINVAL;
    const dim3 grid((uint32_t)(((uint64_t)n + SEG_WAVES - 1) / SEG_WAVES));
    hipLaunchKernelGGL(gather_segments_kernel, grid, dim3(WAVE * SEG_WAVES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(d_src), d_off_in, d_order, d_off_out, static_cast<uint8_t*>(d_dst), n, elem_bytes);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

extern "C" int svx_record_invert(const uint32_t* d_order, uint32_t n, uint32_t* d_rank, void* stream)
{
    if (n == 0) return SVX_OK;
    if (!d_order || !d_rank) return SVX_EINVAL;
    hipLaunchKernelGGL(invert_kernel, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), d_order, d_rank, n);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

extern "C" int svx_record_scatter_segments(const void* d_src, const int64_t* d_src_off, const uint32_t* d_rank, uint32_t rank_lo, uint32_t rank_hi,
                                           const int64_t* d_off_out, int64_t out_base, void* d_dst, uint32_t n, int32_t* d_status, void* stream)
{
    if (rank_lo > rank_hi) return SVX_EINVAL;
    if (n == 0 || rank_lo == rank_hi) return SVX_OK;
    if (!d_src || !d_src_off || !d_rank || !d_off_out || !d_dst || !d_status) return SVX_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_src) & 3u) return SVX_EINVAL;
    const dim3 grid((uint32_t)(((uint64_t)n + SEG_WAVES - 1) / SEG_WAVES));
    hipLaunchKernelGGL(scatter_segments_kernel, grid, dim3(WAVE * SEG_WAVES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(d_src), d_src_off, d_rank, rank_lo, rank_hi, d_off_out, out_base, static_cast<uint8_t*>(d_dst), n, d_status);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

extern "C" int svx_record_retid(void* d_bytes, const int64_t* d_off, uint32_t n, const int32_t* d_map, int32_t n_in, int32_t* d_tid_key,
                                int32_t* d_status, void* stream)
{
    if (n_in < 0) return SVX_EINVAL;
    if (n == 0) return SVX_OK;
    if (!d_bytes || !d_off || !d_status || (n_in > 0 && !d_map)) return SVX_EINVAL;
    const uint64_t blocks = ((uint64_t)n + 255) / 256;
    hipLaunchKernelGGL(record_retid_kernel, dim3((uint32_t)(blocks < RETID_MAX_BLOCKS ? blocks : RETID_MAX_BLOCKS)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), static_cast<uint8_t*>(d_bytes), d_off, n, d_map, n_in, d_tid_key, d_status);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

extern "C" int svx_record_retag_measure(const void* d_bytes, const int64_t* d_off, uint32_t n, const void* d_table, const int32_t* d_table_off,
                                        int32_t m, int64_t* d_new_len, int32_t* d_status, void* stream)
{
    if (m < 0) return SVX_EINVAL;
    if (n == 0 || m == 0) return SVX_OK;
    if (!d_bytes || !d_off || !d_table || !d_table_off || !d_new_len || !d_status) return SVX_EINVAL;
    const svx_recsort::RetagTable table{static_cast<const uint8_t*>(d_table), d_table_off, m};
    const dim3 grid((uint32_t)(((uint64_t)n + SEG_WAVES - 1) / SEG_WAVES));
    hipLaunchKernelGGL(record_retag_measure_kernel, grid, dim3(WAVE * SEG_WAVES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(d_bytes), d_off, n, table, d_new_len, d_status);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

extern "C" int svx_record_retag_write(const void* d_bytes, const int64_t* d_off, uint32_t n, const void* d_table, const int32_t* d_table_off,
                                      int32_t m, const int64_t* d_new_off, void* d_dst, int32_t* d_status, void* stream)
{
    if (m < 0) return SVX_EINVAL;
    if (n == 0 || m == 0) return SVX_OK;
    if (!d_bytes || !d_off || !d_table || !d_table_off || !d_new_off || !d_dst || !d_status) return SVX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_bytes) | reinterpret_cast<uintptr_t>(d_table)) & 3u) return SVX_EINVAL;
    const svx_recsort::RetagTable table{static_cast<const uint8_t*>(d_table), d_table_off, m};
    const dim3 grid((uint32_t)(((uint64_t)n + SEG_WAVES - 1) / SEG_WAVES));
    hipLaunchKernelGGL(record_retag_write_kernel, grid, dim3(WAVE * SEG_WAVES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(d_bytes), d_off, n, table, d_new_off, static_cast<uint8_t*>(d_dst), d_status);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

static_assert(svx_recsort::TAGS_TABLE_WORDS * 4 == SVX_RECORD_TAGS_TABLE_BYTES, "include/svx.h names the table's size");

extern "C" int svx_record_tags_measure(const void* d_bytes, const int64_t* d_off, uint32_t n, const uint32_t* d_table, int64_t* d_new_len,
                                       int32_t* d_status, void* stream)
{
    if (n == 0) return SVX_OK;
    if (!d_bytes || !d_off || !d_table || !d_new_len || !d_status) return SVX_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_table) & 3u) return SVX_EINVAL;
    const dim3 grid((uint32_t)(((uint64_t)n + SEG_WAVES - 1) / SEG_WAVES));
    hipLaunchKernelGGL(record_tags_measure_kernel, grid, dim3(WAVE * SEG_WAVES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(d_bytes), d_off, n, d_table, d_new_len, d_status);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

extern "C" int svx_record_tags_write(const void* d_bytes, const int64_t* d_off, uint32_t n, const uint32_t* d_table, const int64_t* d_new_off,
                                     void* d_dst, int32_t* d_status, void* stream)
{
    if (n == 0) return SVX_OK;
    if (!d_bytes || !d_off || !d_table || !d_new_off || !d_dst || !d_status) return SVX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_bytes) | reinterpret_cast<uintptr_t>(d_table)) & 3u) return SVX_EINVAL;
    const dim3 grid((uint32_t)(((uint64_t)n + SEG_WAVES - 1) / SEG_WAVES));
    hipLaunchKernelGGL(record_tags_write_kernel, grid, dim3(WAVE * SEG_WAVES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t*>(d_bytes), d_off, n, d_table, d_new_off, static_cast<uint8_t*>(d_dst), d_status);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}
