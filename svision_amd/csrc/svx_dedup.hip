// svx_dedup.hip -- one network pass per distinct similarity image of a launch (MI355X, gfx950).
//
// A window's segment-pair records repeat themselves: once the fp64 scaling of svx_raster_common.hpp has mapped two
// records to the same two lines (same reverse flags), read lengths, tags and exact coordinates no longer matter and the
// images are equal bit for bit.  svx_image_dedup keys every record of a launch on its exact line set-up (image_key: the
// two canonical Lines + the reverse flags, 128 bits, no hash), keeps the first occurrence of each key in input order and
// publishes the number of distinct images on the device; the stage kernels' *_live variants then skip the rows behind it
// inside a graph of fixed size, and svx_gather_rows expands the packed results back to one row per input record.
//
//   first_kernel:   a workgroup per 256 records; every lane keys its record, then the workgroup walks the keys of all
//                   earlier tiles (recomputed into LDS: no cross-workgroup dependency) and of its own tile in ascending
//                   order: the first equal key is the record's first occurrence.
//   compact_kernel: one workgroup; an ordered prefix sum over the first-occurrence flags (1024 records per step) gives
//                   every distinct image its compact row, then every record the compact row of its first occurrence.
//   dedup_small_kernel: both steps in one workgroup of the launch's size for up to 1,024 records -- every launch of the
//                   pipeline (64 .. 256 records: 1 .. 4 waves, which find room on a CU that a workgroup of 16 waits for).
// No atomics: the output is the same in every run.
#include "svx_raster_common.hpp"

namespace {

constexpr int KEY_BLOCK = 256, COMPACT_BLOCK = 1024, WAVE = 64;

__device__ inline bool key_eq(const uint4& a, const uint4& b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

__global__ __launch_bounds__(KEY_BLOCK)
void first_kernel(const int32_t* __restrict__ records, uint32_t n, uint32_t* __restrict__ first, uint4* __restrict__ keys)
{
    __shared__ uint4 tile[KEY_BLOCK];
    const uint32_t i = blockIdx.x * KEY_BLOCK + threadIdx.x;
    const uint4 mine = i < n ? svx_raster::image_key(records + (size_t)i * 12) : uint4{0, 0, 0, 0};
    if (keys && i < n) keys[i] = mine;
    uint32_t f = i;
    for (uint32_t t = 0; t <= blockIdx.x; ++t) {
        const uint32_t j0 = t * KEY_BLOCK;
        __syncthreads();                                     // the previous tile is no longer read
        if (t == blockIdx.x) tile[threadIdx.x] = mine;
        else tile[threadIdx.x] = svx_raster::image_key(records + (size_t)(j0 + threadIdx.x) * 12);   // earlier tiles are full
        __syncthreads();
        if (f == i) {                                        // not found yet: the candidates j < i of this tile, ascending
            const uint32_t hi = min((uint32_t)KEY_BLOCK, i - j0);
            for (uint32_t j = 0; j < hi; ++j)
                if (key_eq(tile[j], mine)) { f = j0 + j; break; }
        }
    }
    if (i < n) first[i] = f;
}

// first[] comes in as the first occurrence of every record and leaves as its compact row (d_inv).  The block is the launch
// rounded up to whole waves (at most COMPACT_BLOCK threads): a workgroup of 16 waves waits for a CU with room for all of them.
__global__ __launch_bounds__(COMPACT_BLOCK)
void compact_kernel(const int32_t* __restrict__ records, uint32_t n, uint32_t* __restrict__ inv, uint32_t* __restrict__ row,
                    int32_t* __restrict__ unique, uint32_t* __restrict__ live)
{
    __shared__ uint32_t wave_sum[COMPACT_BLOCK / WAVE];
    __shared__ uint32_t s_base;
    const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    const uint32_t block = blockDim.x;
    if (t == 0) s_base = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n; c0 += block) {
        const uint32_t i = c0 + t;
        const bool is_first = i < n && inv[i] == i;
        const unsigned long long ball = __ballot(is_first);
        const uint32_t below = __popcll(ball & ((1ull << lane) - 1ull));
        if (lane == 0) wave_sum[wv] = __popcll(ball);
        __syncthreads();
        uint32_t before = s_base;
        for (int w = 0; w < wv; ++w) before += wave_sum[w];
        if (is_first) {
            const uint32_t c = before + below;
            row[i] = c;
#pragma unroll
            for (int e = 0; e < 12; ++e) unique[(size_t)c * 12 + e] = records[(size_t)i * 12 + e];
        }
        __syncthreads();                                     // every lane has read s_base and wave_sum
        if (t == 0) { uint32_t s = s_base; for (uint32_t w = 0; w < block / WAVE; ++w) s += wave_sum[w]; s_base = s; }
        __syncthreads();
    }
    const uint32_t n_live = s_base;
    // rows behind the distinct images repeat the first record: a consumer without the live count computes a valid image there
    for (uint32_t e = n_live * 12 + t; e < n * 12; e += block) unique[e] = records[e % 12];
    for (uint32_t i = t; i < n; i += block) inv[i] = row[inv[i]];
    if (t == 0) *live = n_live;
}

// Both steps in one workgroup for a launch of at most COMPACT_BLOCK records (every launch of the pipeline): a lane per record
// keys it, walks the keys in front of it in ascending order, and the ordered prefix sum over the first-occurrence flags gives
// the compact rows -- the same outputs as first_kernel + compact_kernel, without the second launch and its scratch.
__global__ __launch_bounds__(COMPACT_BLOCK)
void dedup_small_kernel(const int32_t* __restrict__ records, uint32_t n, uint32_t* __restrict__ inv, int32_t* __restrict__ unique,
                        uint32_t* __restrict__ live, uint4* __restrict__ keys)
{
    constexpr uint32_t SCAN = 8;                             // divides the block: a turn never reads behind it
    __shared__ uint4 tile[COMPACT_BLOCK];
    __shared__ uint32_t row[COMPACT_BLOCK];
    __shared__ uint32_t wave_sum[COMPACT_BLOCK / WAVE];
    const uint32_t i = threadIdx.x, lane = i & (WAVE - 1), wv = i / WAVE, block = blockDim.x;
    const uint4 mine = i < n ? svx_raster::image_key(records + (size_t)i * 12) : uint4{0, 0, 0, 0};
    if (keys && i < n) keys[i] = mine;
    tile[i] = mine;
    __syncthreads();
    uint32_t f = i;
    if (i < n)
        for (uint32_t j0 = 0; j0 < i && f == i; j0 += SCAN) {  // SCAN keys per turn, their loads in flight together: the first equal one
            uint32_t hit = 0;
#pragma unroll
            for (uint32_t u = 0; u < SCAN; ++u)
                if (key_eq(tile[j0 + u], mine) && j0 + u < i) hit |= 1u << u;
            if (hit) f = j0 + __ffs(hit) - 1;
        }
    const bool is_first = i < n && f == i;
    const unsigned long long ball = __ballot(is_first);
    const uint32_t below = __popcll(ball & ((1ull << lane) - 1ull));
    if (lane == 0) wave_sum[wv] = __popcll(ball);
    __syncthreads();
    uint32_t before = 0, n_live = 0;
    for (uint32_t w = 0; w < block / WAVE; ++w) { if (w == wv) before = n_live; n_live += wave_sum[w]; }
    if (is_first) {
        const uint32_t c = before + below;
        row[i] = c;
#pragma unroll
        for (int e = 0; e < 12; ++e) unique[(size_t)c * 12 + e] = records[(size_t)i * 12 + e];
    }
    __syncthreads();
    if (i < n) inv[i] = row[f];
    for (uint32_t e = n_live * 12 + i; e < n * 12; e += block) unique[e] = records[e % 12];
    if (i == 0) *live = n_live;
}

__global__ __launch_bounds__(256)
void gather_rows_kernel(const float* __restrict__ src, const uint32_t* __restrict__ inv, float* __restrict__ dst, uint32_t n, uint32_t width)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n * width) return;
    const uint32_t i = e / width, c = e - i * width;
    dst[e] = src[(size_t)inv[i] * width + c];
}

}  // namespace

extern "C" int svx_image_dedup(const int32_t* d_records, uint32_t n, int32_t* d_unique, uint32_t* d_inv, uint32_t* d_live,
                               uint32_t* d_keys, uint32_t* d_ws, void* stream)
{
    if (!d_live) return SVX_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n == 0) return hipMemsetAsync(d_live, 0, sizeof(uint32_t), st) == hipSuccess ? SVX_OK : SVX_ELAUNCH;
    if (!d_records || !d_unique || !d_inv || !d_ws || n > (1u << 26)) return SVX_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_keys) & 15u) return SVX_EINVAL;
    const uint32_t block = n >= COMPACT_BLOCK ? COMPACT_BLOCK : (n + WAVE - 1) / WAVE * WAVE;
    if (n <= COMPACT_BLOCK) {
        hipLaunchKernelGGL(dedup_small_kernel, dim3(1), dim3(block), 0, st, d_records, n, d_inv, d_unique, d_live, reinterpret_cast<uint4*>(d_keys));
        return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
    }
    hipLaunchKernelGGL(first_kernel, dim3((n + KEY_BLOCK - 1) / KEY_BLOCK), dim3(KEY_BLOCK), 0, st, d_records, n, d_inv,
                       reinterpret_cast<uint4*>(d_keys));
    hipLaunchKernelGGL(compact_kernel, dim3(1), dim3(block), 0, st, d_records, n, d_inv, d_ws, d_unique, d_live);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

extern "C" int svx_gather_rows(const float* d_src, const uint32_t* d_inv, float* d_dst, uint32_t n, uint32_t width, void* stream)
{
    if (n == 0 || width == 0) return SVX_OK;
    if (!d_src || !d_inv || !d_dst || (uint64_t)n * width > 0xffffffffull) return SVX_EINVAL;
    const uint32_t total = n * width;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), d_src, d_inv, d_dst, n, width);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}
