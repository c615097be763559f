// svx_deflate.hip -- BGZF members from inflated bytes on gfx950: the DEFLATE encoder the ingest path lacked (svision_amd/sort.py
// writes a device-sorted BAM with it).
//
// bgzf_deflate_kernel   one WORKGROUP per block of 0 .. 0xFF00 bytes, block and hash table in LDS (153 KB of the CU's 160 KB):
//                       hash -> match -> parse -> bits per tile of 1,024 positions, all of it in svx_deflate_core.hpp (the phases, and
//                       why the member is a pure function of the input).  Fixed Huffman code, or stored where that is not smaller.
//                       Member b goes to slot b of 65,536 bytes
// bgzf_deflate_dyn_kernel the same parse with its tokens kept in a global workspace and counted in LDS, then the smallest of stored, fixed
//                       and DYNAMIC Huffman codes built in the workgroup (BTYPE 10; svx_deflate_core.hpp, encode_block_dyn); 1,280 bytes
//                       of LDS more for the histograms, the code construction in the LDS the hash table has left
// bgzf_crc32_put_kernel (svx_crc.hip) the CRC32 of the input block into the member's footer: the device function svx_bgzf_crc32 checks with
// member_offsets_kernel exclusive prefix sum of the members' lengths, one workgroup
// bgzf_pack_kernel      the members from their slots to their offsets: contiguous file bytes
// No communication between workgroups; the LDS atomics are max, or and integer add, whose results do not depend on the order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "../../include/svx.h"
#include "svx_deflate_core.hpp"

extern "C" __attribute__((visibility("hidden"))) int svx_bgzf_crc32_put(const uint8_t* d_in, const uint64_t* d_in_off, uint32_t n_blocks, uint8_t* d_slots, uint32_t slot_bytes,
                                  const uint32_t* d_member_len, void* stream);

namespace {

constexpr uint32_t DFL_LDS = svx_dfl::LDS_BYTES + svx_dfl::WAVES * sizeof(uint32_t);
constexpr uint32_t DYN_LDS = svx_dfl::DYN_LDS_BYTES + svx_dfl::WAVES * sizeof(uint32_t);
constexpr uint32_t DYN_TICKS = 4;                    // clock readings a block that a workspace with room for them receives
constexpr int PACK_THREADS = 256, SCAN_THREADS = 1024;

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)v, o, 64); if (lane >= o) v += u; }
    return v;
}

// the workgroup as svx_dfl::encode_block sees it
struct Workgroup {
    uint32_t* part;                                  // [WAVES] in LDS
    uint64_t* ticks = nullptr;                       // [DYN_TICKS] of the block, or none
    __device__ __forceinline__ void tick(uint32_t k) { if (ticks && threadIdx.x == 0) ticks[k] = wall_clock64(); }
    __device__ __forceinline__ void atomic_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
    template <class F> __device__ __forceinline__ void each(F f) { f(threadIdx.x); }
    __device__ __forceinline__ void barrier() { __syncthreads(); }
    __device__ __forceinline__ void wave_sync() { __builtin_amdgcn_wave_barrier(); }
    __device__ __forceinline__ void atomic_max(uint32_t* p, uint32_t v) { atomicMax(p, v); }
    __device__ __forceinline__ void atomic_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
    __device__ __forceinline__ void scan(uint32_t* a, uint32_t* total)
    {
        const uint32_t t = threadIdx.x;
        const int lane = (int)(t & 63u), wave = (int)(t >> 6);
        __syncthreads();
        const uint32_t v = a[t], incl = wave_incl_sum(v, lane);
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < (int)svx_dfl::WAVES; ++k) { const uint32_t s = part[k]; all += s; if (k < wave) before += s; }
        a[t] = before + incl - v;
        __syncthreads();                             // (also keeps the next scan's sums out of `part` until everybody has read these)
        *total = all;
    }
};

__global__ __launch_bounds__(svx_dfl::T)
void bgzf_deflate_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off, uint32_t n_blocks, uint8_t* __restrict__ slots,
                         uint32_t* __restrict__ member_len, uint32_t* __restrict__ stored)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t dfl_lds[];
    const uint32_t b = blockIdx.x;
    const uint64_t lo = in_off[b], hi = in_off[b + 1];
    if (hi < lo || hi - lo > svx_dfl::MAX_IN) {      // (uniform) not a block this encoder takes: no member, the entry point's caller sees length 0
        if (threadIdx.x == 0) { member_len[b] = 0; stored[b] = 0; }
        return;
    }
    const svx_dfl::Ctx c = svx_dfl::carve(dfl_lds);
    Workgroup wg{reinterpret_cast<uint32_t*>(dfl_lds + svx_dfl::LDS_BYTES)};
    svx_dfl::encode_block(wg, c, in + lo, (uint32_t)(hi - lo), slots + (uint64_t)b * svx_dfl::SLOT, member_len + b, stored + b);
}

// ws: n_blocks x WS_BLOCK bytes of tokens and marks; ticks: n_blocks x DYN_TICKS clock readings, or null
__global__ __launch_bounds__(svx_dfl::T)
void bgzf_deflate_dyn_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off, uint32_t n_blocks, uint8_t* __restrict__ slots,
                             uint32_t* __restrict__ member_len, uint32_t* __restrict__ btype, uint8_t* ws, uint64_t* ticks)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t dfl_lds[];
    const uint32_t b = blockIdx.x;
    const uint64_t lo = in_off[b], hi = in_off[b + 1];
    if (hi < lo || hi - lo > svx_dfl::MAX_IN) {      // (uniform) as bgzf_deflate_kernel
        if (threadIdx.x == 0) { member_len[b] = 0; btype[b] = 0; }
        return;
    }
    const svx_dfl::Ctx c = svx_dfl::carve(dfl_lds);
    const svx_dfl::DynCtx d = svx_dfl::carve_dyn(dfl_lds, c, ws + (uint64_t)b * svx_dfl::WS_BLOCK);
    Workgroup wg{reinterpret_cast<uint32_t*>(dfl_lds + svx_dfl::DYN_LDS_BYTES), ticks ? ticks + (uint64_t)b * DYN_TICKS : nullptr};
    svx_dfl::encode_block_dyn(wg, c, d, in + lo, (uint32_t)(hi - lo), slots + (uint64_t)b * svx_dfl::SLOT, member_len + b, btype + b);
}

// file_off [n + 1] = exclusive prefix sum of member_len [n], the closing entry = the file bytes
__global__ __launch_bounds__(SCAN_THREADS)
void member_offsets_kernel(const uint32_t* __restrict__ member_len, uint32_t n, uint64_t* __restrict__ file_off)
{
    __shared__ uint32_t part[SCAN_THREADS / 64];
    const uint32_t t = threadIdx.x;
    const int lane = (int)(t & 63u), wave = (int)(t >> 6);
    uint64_t run = 0;                                // (uniform) the bytes of the batches in front
    for (uint32_t i0 = 0; i0 < n; i0 += SCAN_THREADS) {
        const uint32_t v = i0 + t < n ? member_len[i0 + t] : 0u, incl = wave_incl_sum(v, lane);
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int k = 0; k < SCAN_THREADS / 64; ++k) { const uint32_t s = part[k]; all += s; if (k < wave) before += s; }
        if (i0 + t < n) file_off[i0 + t] = run + before + incl - v;
        run += all;
        __syncthreads();
    }
    if (t == 0) file_off[n] = run;
}

__global__ __launch_bounds__(PACK_THREADS)
void bgzf_pack_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ member_len, const uint64_t* __restrict__ file_off,
                      uint8_t* __restrict__ out, uint64_t out_bytes)
{
    const uint32_t b = blockIdx.x, len = member_len[b];
    const uint64_t at = file_off[b];
    if (len > svx_dfl::SLOT || at + len > out_bytes) return;      // (uniform) no room: the entry point's caller compares file_off[n] with out_bytes
    const uint8_t* src = slots + (uint64_t)b * svx_dfl::SLOT;
    for (uint32_t i = threadIdx.x; i < len; i += PACK_THREADS) out[at + i] = src[i];
}

constexpr int KEPT = 64;

// The LDS limit and the kernel's dynamic-LDS opt-in belong to the CURRENT device: the answer is kept per device (0 not asked yet,
// 1 ready, 2 no room).  Two threads that ask at once both set the attribute, to the same value.
template <class K>
int kernel_ready(K kernel, uint32_t lds_bytes, std::atomic<int>* state)
{
    int dev = 0, max_lds = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    const bool kept = dev >= 0 && dev < KEPT;
    if (kept) { const int s = state[dev].load(std::memory_order_acquire); if (s) return s == 1; }
    int ok = 0;
    if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && (uint32_t)max_lds >= lds_bytes)
        ok = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) == hipSuccess;
    if (kept) state[dev].store(ok ? 1 : 2, std::memory_order_release);
    return ok;
}

int deflate_ready()
{
    static std::atomic<int> state[KEPT];
    return kernel_ready(bgzf_deflate_kernel, DFL_LDS, state);
}

int deflate_dyn_ready()
{
    static std::atomic<int> state[KEPT];
    return kernel_ready(bgzf_deflate_dyn_kernel, DYN_LDS, state);
}

}  // namespace

extern "C" int svx_bgzf_deflate(const uint8_t* d_in, const uint64_t* d_in_off, uint32_t n_blocks, uint8_t* d_slots, uint32_t* d_member_len,
                                uint32_t* d_stored, void* stream)
{
    if (n_blocks == 0) return SVX_OK;
    if (!d_in || !d_in_off || !d_slots || !d_member_len || !d_stored) return SVX_EINVAL;
    if (!deflate_ready()) return SVX_ELAUNCH;
    hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(n_blocks), dim3(svx_dfl::T), DFL_LDS, static_cast<hipStream_t>(stream),
                       d_in, d_in_off, n_blocks, d_slots, d_member_len, d_stored);
    if (hipGetLastError() != hipSuccess) return SVX_ELAUNCH;
    return svx_bgzf_crc32_put(d_in, d_in_off, n_blocks, d_slots, svx_dfl::SLOT, d_member_len, stream);
}

extern "C" size_t svx_bgzf_deflate_dyn_ws_bytes(uint32_t n_blocks) { return (size_t)n_blocks * svx_dfl::WS_BLOCK; }

extern "C" int svx_bgzf_deflate_dyn(const uint8_t* d_in, const uint64_t* d_in_off, uint32_t n_blocks, uint8_t* d_slots, uint32_t* d_member_len,
                                    uint32_t* d_btype, void* d_ws, uint64_t ws_bytes, void* stream)
{
    if (n_blocks == 0) return SVX_OK;
    if (!d_in || !d_in_off || !d_slots || !d_member_len || !d_btype || !d_ws || (reinterpret_cast<uintptr_t>(d_ws) & 7u)) return SVX_EINVAL;
    const uint64_t need = (uint64_t)n_blocks * svx_dfl::WS_BLOCK;
    if (ws_bytes < need) return SVX_ECAPACITY;
    if (!deflate_dyn_ready()) return SVX_ELAUNCH;
    // (the phases' clock readings for tools/sort_write_time.py: only into a workspace that has 32 bytes a block to spare)
    uint64_t* ticks = ws_bytes >= need + (uint64_t)n_blocks * DYN_TICKS * sizeof(uint64_t) ? reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_ws) + need) : nullptr;
    hipLaunchKernelGGL(bgzf_deflate_dyn_kernel, dim3(n_blocks), dim3(svx_dfl::T), DYN_LDS, static_cast<hipStream_t>(stream),
                       d_in, d_in_off, n_blocks, d_slots, d_member_len, d_btype, static_cast<uint8_t*>(d_ws), ticks);
    if (hipGetLastError() != hipSuccess) return SVX_ELAUNCH;
    return svx_bgzf_crc32_put(d_in, d_in_off, n_blocks, d_slots, svx_dfl::SLOT, d_member_len, stream);
}

extern "C" int svx_bgzf_pack(const uint8_t* d_slots, const uint32_t* d_member_len, uint32_t n_blocks, uint64_t* d_file_off, uint8_t* d_out,
                             uint64_t out_bytes, void* stream)
{
    if (!d_file_off) return SVX_EINVAL;
    if (n_blocks && (!d_slots || !d_member_len || !d_out)) return SVX_EINVAL;
    hipLaunchKernelGGL(member_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, static_cast<hipStream_t>(stream), d_member_len, n_blocks, d_file_off);
    if (hipGetLastError() != hipSuccess) return SVX_ELAUNCH;
    if (n_blocks == 0) return SVX_OK;
    hipLaunchKernelGGL(bgzf_pack_kernel, dim3(n_blocks), dim3(PACK_THREADS), 0, static_cast<hipStream_t>(stream),
                       d_slots, d_member_len, d_file_off, d_out, out_bytes);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}
