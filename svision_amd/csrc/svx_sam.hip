// svx_sam.hip -- SAM text -> BAM records on gfx950: the front end of svision_amd/sort.py for an aligner's text output.  The phases
// are svx_sam_core.hpp's (the rules: svision_amd/io/sam.py); here are the launches.
//
// sam_count_kernel     a workgroup a tile of 4,096 bytes, a thread 16 of them: the tile's newlines
// sam_tile_scan_kernel ONE workgroup: the exclusive prefix of the tiles' counts, the number of lines
// sam_emit_kernel      the tile again: a thread's newlines, ranked by the tile's base + the workgroup's prefix -> line_off
// sam_measure_kernel   a WAVE a line: the record's bytes or a negative code, and tid pos flag span
// sam_encode_kernel    a WAVE a line: the record at its offset
// sam_pack_count_kernel / sam_pack_extract_kernel
//                      a WAVE a line, a bounded grid whose waves stride over the lines: the line's fields and the sizes of its CIGAR
//                      words, name and SEQ; then those written into the caller's packed arrays (no BAM record in between)
// No atomics, no communication between workgroups, no spin-wait; a wave's lanes meet in ballots and shuffles only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/svx.h"
#include "svx_sam_core.hpp"

namespace {

constexpr int WAVES = 4;                                        // lines a workgroup of the record kernels
constexpr int SCAN_THREADS = 1024;

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64); if (lane >= o) v += u; }
    return v;
}

// the wave as svx_sam::record sees it
struct Wave {
    uint32_t lane;
    template <class F> __device__ __forceinline__ void each(F f) { f(lane); }
    template <class F> __device__ __forceinline__ uint64_t ballot(F f) { return __ballot(f(lane) ? 1 : 0); }
    template <class F> __device__ __forceinline__ uint64_t sum(F f)
    {
        uint64_t v = f(lane);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
        return (uint64_t)hi << 32 | lo;                          // (the same in every lane: kept where uniform values live)
    }
};

__global__ __launch_bounds__(svx_sam::THREADS)
void sam_count_kernel(const uint8_t* __restrict__ text, uint64_t n, uint32_t* __restrict__ tile_count)
{
    __shared__ uint32_t part[svx_sam::THREADS / 64];
    const uint32_t t = threadIdx.x;
    const int lane = (int)(t & 63u), wave = (int)(t >> 6);
    const uint32_t incl = wave_incl_sum(svx_sam::count_newlines(text, n, blockIdx.x, t), lane);
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    if (t == 0) { uint32_t all = 0; for (int k = 0; k < (int)svx_sam::THREADS / 64; ++k) all += part[k]; tile_count[blockIdx.x] = all; }
}

// tile_base [n_tiles] = exclusive prefix of tile_count; *n_lines = the newlines + 1 where the last byte is none; line_off[0] = 0 and,
// for that unclosed last line, line_off[n_lines] = n
__global__ __launch_bounds__(SCAN_THREADS)
void sam_tile_scan_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ tile_count, uint32_t n_tiles,
                          uint64_t* __restrict__ tile_base, int64_t* __restrict__ line_off, uint64_t cap, uint64_t* __restrict__ n_lines)
{
    __shared__ uint32_t part[SCAN_THREADS / 64];
    const uint32_t t = threadIdx.x;
    const int lane = (int)(t & 63u), wave = (int)(t >> 6);
    uint64_t run = 0;
    for (uint32_t i0 = 0; i0 < n_tiles; i0 += SCAN_THREADS) {
        const uint32_t v = i0 + t < n_tiles ? tile_count[i0 + t] : 0u, incl = wave_incl_sum(v, lane);
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int k = 0; k < SCAN_THREADS / 64; ++k) { const uint32_t s = part[k]; all += s; if (k < wave) before += s; }
        if (i0 + t < n_tiles) tile_base[i0 + t] = run + before + incl - v;
        run += all;
        __syncthreads();
    }
    if (t == 0) {
        const bool open = n > 0 && text[n - 1] != '\n';
        *n_lines = run + open;
        if (cap > 0) line_off[0] = 0;
        if (open && run + 1 < cap) line_off[run + 1] = (int64_t)n;
    }
}

__global__ __launch_bounds__(svx_sam::THREADS)
void sam_emit_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint64_t* __restrict__ tile_base, int64_t* __restrict__ line_off, uint64_t cap)
{
    __shared__ uint32_t part[svx_sam::THREADS / 64];
    const uint32_t t = threadIdx.x;
    const int lane = (int)(t & 63u), wave = (int)(t >> 6);
    const uint32_t v = svx_sam::count_newlines(text, n, blockIdx.x, t), incl = wave_incl_sum(v, lane);
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (int k = 0; k < wave; ++k) before += part[k];
    svx_sam::emit_newlines(text, n, blockIdx.x, t, tile_base[blockIdx.x] + before + incl - v, line_off, cap);
}

__global__ __launch_bounds__(WAVES * 64)
void sam_measure_kernel(const uint8_t* __restrict__ text, const int64_t* __restrict__ line_off, uint32_t n_lines, svx_sam::RefTable rt,
                        int32_t* __restrict__ len, int32_t* __restrict__ tid, int32_t* __restrict__ pos, int32_t* __restrict__ flag,
                        int32_t* __restrict__ span)
{
    const uint64_t i = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n_lines) return;                                   // (whole waves leave)
    Wave w{threadIdx.x & 63u};
    svx_sam::measure_line(w, text, line_off, i, rt, len, tid, pos, flag, span);
}

__global__ __launch_bounds__(WAVES * 64)
void sam_encode_kernel(const uint8_t* __restrict__ text, const int64_t* __restrict__ line_off, uint32_t n_lines, svx_sam::RefTable rt,
                       const int32_t* __restrict__ len, const int64_t* __restrict__ off, int64_t out_base, uint8_t* __restrict__ out,
                       int32_t* __restrict__ status)
{
    const uint64_t i = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n_lines) return;
    Wave w{threadIdx.x & 63u};
    svx_sam::encode_line(w, text, line_off, i, rt, len, off, out_base, out, status);
}

// the pack kernels' grid: at most PACK_BLOCKS workgroups, every wave takes the lines i, i + the grid's waves, ...
constexpr uint32_t PACK_BLOCKS = 4096;

__global__ __launch_bounds__(WAVES * 64)
void sam_pack_count_kernel(const uint8_t* __restrict__ text, const int64_t* __restrict__ line_off, uint32_t n_lines, svx_sam::RefTable rt,
                           int with_seq, int32_t* __restrict__ status, int32_t* __restrict__ fields, int32_t* __restrict__ counts)
{
    Wave w{threadIdx.x & 63u};
    for (uint64_t i = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); i < n_lines; i += (uint64_t)gridDim.x * WAVES)   // (whole waves leave)
        svx_sam::pack_count_line(w, text, line_off, i, n_lines, rt, with_seq != 0, status, fields, counts);
}

__global__ __launch_bounds__(WAVES * 64)
void sam_pack_extract_kernel(const uint8_t* __restrict__ text, const int64_t* __restrict__ line_off, uint32_t n_lines, svx_sam::RefTable rt,
                             const int32_t* __restrict__ status, svx_sam::PackOut out)
{
    Wave w{threadIdx.x & 63u};
    for (uint64_t i = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); i < n_lines; i += (uint64_t)gridDim.x * WAVES)
        svx_sam::pack_extract_line(w, text, line_off, i, rt, status, out);
}

inline uint32_t pack_grid(uint32_t n_lines) { const uint32_t b = (n_lines + WAVES - 1) / WAVES; return b < PACK_BLOCKS ? b : PACK_BLOCKS; }

inline uint64_t tiles_of(uint64_t n) { return (n + svx_sam::TILE - 1) / svx_sam::TILE; }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int launched() { return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH; }

}  // namespace

extern "C" size_t svx_sam_lines_ws_bytes(uint64_t n_bytes)
{
    const uint64_t tiles = tiles_of(n_bytes) + 1;
    return align256(tiles * sizeof(uint32_t)) + align256(tiles * sizeof(uint64_t));
}

extern "C" int svx_sam_lines(const uint8_t* d_text, uint64_t n_bytes, int64_t* d_line_off, uint64_t cap, uint64_t* d_n_lines, void* d_ws,
                             uint64_t ws_bytes, void* stream)
{
    const uint64_t tiles = tiles_of(n_bytes);
    if (!d_text || !d_line_off || !d_n_lines || !d_ws || cap < 1 || tiles > 0x7FFFFFFFu) return SVX_EINVAL;
    if (ws_bytes < svx_sam_lines_ws_bytes(n_bytes)) return SVX_ECAPACITY;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* tile_count = static_cast<uint32_t*>(d_ws);
    uint64_t* tile_base = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_ws) + align256((tiles + 1) * sizeof(uint32_t)));
    if (tiles) hipLaunchKernelGGL(sam_count_kernel, dim3((uint32_t)tiles), dim3(svx_sam::THREADS), 0, st, d_text, n_bytes, tile_count);
    hipLaunchKernelGGL(sam_tile_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, d_text, n_bytes, tile_count, (uint32_t)tiles, tile_base, d_line_off,
                       cap, d_n_lines);
    if (tiles) hipLaunchKernelGGL(sam_emit_kernel, dim3((uint32_t)tiles), dim3(svx_sam::THREADS), 0, st, d_text, n_bytes, tile_base, d_line_off, cap);
    return launched();
}

extern "C" int svx_sam_measure(const uint8_t* d_text, const int64_t* d_line_off, uint32_t n_lines, const uint32_t* d_ref_hash,
                               const int32_t* d_ref_tid, const uint32_t* d_ref_name_off, const uint8_t* d_ref_names, uint32_t n_ref,
                               int32_t* d_len, int32_t* d_tid, int32_t* d_pos, int32_t* d_flag, int32_t* d_span, void* stream)
{
    if (n_lines == 0) return SVX_OK;
    if (!d_text || !d_line_off || !d_ref_hash || !d_ref_tid || !d_ref_name_off || !d_ref_names || !d_len || !d_tid || !d_pos || !d_flag || !d_span)
        return SVX_EINVAL;
    const svx_sam::RefTable rt{d_ref_hash, d_ref_tid, d_ref_name_off, d_ref_names, n_ref};
    hipLaunchKernelGGL(sam_measure_kernel, dim3((n_lines + WAVES - 1) / WAVES), dim3(WAVES * 64), 0, static_cast<hipStream_t>(stream), d_text,
                       d_line_off, n_lines, rt, d_len, d_tid, d_pos, d_flag, d_span);
    return launched();
}

extern "C" int svx_sam_encode(const uint8_t* d_text, const int64_t* d_line_off, uint32_t n_lines, const uint32_t* d_ref_hash,
                              const int32_t* d_ref_tid, const uint32_t* d_ref_name_off, const uint8_t* d_ref_names, uint32_t n_ref,
                              const int32_t* d_len, const int64_t* d_off, int64_t out_base, uint8_t* d_out, int32_t* d_status, void* stream)
{
    if (n_lines == 0) return SVX_OK;
    if (!d_text || !d_line_off || !d_ref_hash || !d_ref_tid || !d_ref_name_off || !d_ref_names || !d_len || !d_off || !d_out || !d_status)
        return SVX_EINVAL;
    const svx_sam::RefTable rt{d_ref_hash, d_ref_tid, d_ref_name_off, d_ref_names, n_ref};
    hipLaunchKernelGGL(sam_encode_kernel, dim3((n_lines + WAVES - 1) / WAVES), dim3(WAVES * 64), 0, static_cast<hipStream_t>(stream), d_text,
                       d_line_off, n_lines, rt, d_len, d_off, out_base, d_out, d_status);
    return launched();
}

extern "C" int svx_sam_pack_count(const uint8_t* d_text, const int64_t* d_line_off, uint32_t n_lines, const uint32_t* d_ref_hash,
                                  const int32_t* d_ref_tid, const uint32_t* d_ref_name_off, const uint8_t* d_ref_names, uint32_t n_ref,
                                  int with_seq, int32_t* d_status, int32_t* d_fields, int32_t* d_counts, void* stream)
{
    if (n_lines == 0) return SVX_OK;
    if (!d_text || !d_line_off || !d_ref_hash || !d_ref_tid || !d_ref_name_off || !d_ref_names || !d_status || !d_fields || !d_counts) return SVX_EINVAL;
    const svx_sam::RefTable rt{d_ref_hash, d_ref_tid, d_ref_name_off, d_ref_names, n_ref};
    hipLaunchKernelGGL(sam_pack_count_kernel, dim3(pack_grid(n_lines)), dim3(WAVES * 64), 0, static_cast<hipStream_t>(stream), d_text, d_line_off,
                       n_lines, rt, with_seq, d_status, d_fields, d_counts);
    return launched();
}

extern "C" int svx_sam_pack_extract(const uint8_t* d_text, const int64_t* d_line_off, uint32_t n_lines, const uint32_t* d_ref_hash,
                                    const int32_t* d_ref_tid, const uint32_t* d_ref_name_off, const uint8_t* d_ref_names, uint32_t n_ref,
                                    const int32_t* d_status, int32_t* d_tid, int32_t* d_pos, int16_t* d_flag, uint8_t* d_mapq, int32_t* d_l_seq,
                                    const int64_t* d_cig_off, uint32_t* d_cigar, const int64_t* d_name_off, uint8_t* d_names,
                                    const int64_t* d_seq_off, uint8_t* d_seq, void* stream)
{
    if (n_lines == 0) return SVX_OK;
    if (!d_text || !d_line_off || !d_ref_hash || !d_ref_tid || !d_ref_name_off || !d_ref_names || !d_status || !d_tid || !d_pos || !d_flag || !d_mapq
        || !d_l_seq || !d_cig_off || !d_cigar || !d_name_off || !d_names || (d_seq != nullptr) != (d_seq_off != nullptr))
        return SVX_EINVAL;
    const svx_sam::RefTable rt{d_ref_hash, d_ref_tid, d_ref_name_off, d_ref_names, n_ref};
    const svx_sam::PackOut out{d_tid, d_pos, d_l_seq, d_flag, d_mapq, d_cig_off, d_cigar, d_name_off, d_names, d_seq_off, d_seq};
    hipLaunchKernelGGL(sam_pack_extract_kernel, dim3(pack_grid(n_lines)), dim3(WAVES * 64), 0, static_cast<hipStream_t>(stream), d_text, d_line_off,
                       n_lines, rt, d_status, out);
    return launched();
}
