// svx_lz_table.hip -- the LZ77 copies of a BGZF block by pointer doubling in LDS, one WORKGROUP per block (gfx950: the table
// of a 65,280-byte block is 127.5 KB of the CU's 160 KB).
//
// bgzf_lz_kernel (one lane per block) walks a block's ~9,500 sequences one after the other: 25 ms whatever the launch holds.
// bgzf_lz_wave_kernel executes them in order, all lanes on a few: ~0.5-1 ms per block.  Here nothing is in order
// (svx_lz_table_core.hpp: the table, the phases and why they are right):
//   build    batches of LZT_THREADS sequences, one thread each: two workgroup prefix sums give every sequence its output and
//            literal offsets; the batch is validated in uniform control flow (output or literal overrun, a distance beyond the
//            block's start -- the block's status is set and the workgroup leaves); then every thread writes its sequence's
//            entries: literals as values, match bytes as pointers to their source positions.  What a batch reads is on its way
//            before the batch needs it: the block's literals are touched once, a cache line per thread, in front of the first
//            batch, and a batch's headers are loaded while the batch in front of it is written
//   resolve  rounds of entry = table[entry] over all entries, in place, until no pointer is left (__syncthreads_or; at most
//            MAX_ROUNDS rounds -- the cap is what guarantees the kernel ends, whatever the table holds)
//   emit     16 entries = one aligned 16-byte store; the output is written once and never read
// No communication between workgroups, no atomics, no spin waits.  A block of more than 0xFF00 bytes cannot take the table: its
// status becomes `handover` and the entry point gives it to the wave-per-block inflater, as it does with the blocks whose
// sequence stream did not fit its slot.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/svx.h"
#include "svx_lz_table_core.hpp"
#include "svx_wave_scan.hpp"

#ifndef SVX_LZT_DBG
#define SVX_LZT_DBG 0                // measurements only (wrong output): 1 = leave behind the build, 2 = no literal entries, 4 = no match entries
#endif

namespace {

#ifndef SVX_LZT_THREADS
#define SVX_LZT_THREADS 1024
#endif
constexpr int LZT_THREADS = SVX_LZT_THREADS, LZT_WAVES = LZT_THREADS / 64;
static_assert(LZT_WAVES <= 64, "the waves' sums are scanned by one wave's lanes");
constexpr uint32_t LZT_LDS = svx_lzt::TABLE_BYTES + 2u * LZT_WAVES * sizeof(uint32_t);      // [table][the waves' sums of the batch: output, literals]

constexpr uint32_t LZT_PARTS = 3u & ~((uint32_t)SVX_LZT_DBG >> 1);      // the parts of a sequence the build writes (all, but in a measurement build)

__global__ __launch_bounds__(LZT_THREADS)
void bgzf_lz_table_kernel(const uint8_t* __restrict__ streams, const uint2* __restrict__ stream_cnt, const uint64_t* __restrict__ dst_off,
                          uint32_t n_blocks, uint8_t* out, uint32_t* status, uint32_t handover)
{
    // (dynamic: with static LDS the compiler raises the VGPR allocation to what the LDS-limited occupancy leaves room for --
    // svx_inflate2.hip, bgzf_lz_kernel)
    extern __shared__ __attribute__((aligned(16))) uint8_t lzt_lds[];
    uint16_t* const tab = reinterpret_cast<uint16_t*>(lzt_lds);
    uint32_t* const part = reinterpret_cast<uint32_t*>(lzt_lds + svx_lzt::TABLE_BYTES);
    const uint32_t b = blockIdx.x, t = threadIdx.x;
    const int lane = (int)(t & 63u), wave = (int)(t >> 6);
    // (everything the block's addresses depend on in one round trip, not one load behind the other)
    const uint32_t st0 = status[b];                      // (nobody writes it before the first barrier below)
    const uint64_t lo = dst_off[b], hi = dst_off[b + 1], first_off = dst_off[0];
    const uint2 cnt = stream_cnt[b];
    if (st0 != 0) return;
    if (hi == lo) return;
    if (hi - lo > svx_lzt::MAX_OUT) {                    // not for the table: the entry point hands the block over
        __syncthreads();
        if (t == 0) status[b] = handover;
        return;
    }
    const uint32_t isize = (uint32_t)(hi - lo), ph = (uint32_t)lo & 15u;
    const uint32_t nseq = cnt.x, nlit = cnt.y;
    const uint64_t slot_lo = svx_lzt::slot_at(lo - first_off, b), slot_hi = svx_lzt::slot_at(hi - first_off, b + 1);
    const uint8_t* slot = streams + slot_lo;
    const uint8_t* lit_end = streams + slot_hi;
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(slot + ((uint32_t)(-(intptr_t)reinterpret_cast<uintptr_t>(slot)) & 3u));
    // ---- build
    if (t < 32u) svx_lzt::pad_write(tab, ph, isize, t);
    uint32_t W = 0, L = 0;                               // (uniform) output and literal bytes of the batches in front
    int err = svx_lzt::LZ_OK;
    // The block's literals lie in [lit_end - nlit, lit_end), inside its slot: one byte of every 64 is read here, by all threads at
    // once, so that the batches' literal loads find their lines on the way or in the cache (the sum is used only to keep the
    // loads: nothing waits for it before the build is over).  Never outside the slot, whatever nlit says.
    uint32_t warm = 0;
    {
        const uint64_t room = slot_hi - slot_lo;
        const uint32_t span = nlit < room ? nlit : (uint32_t)room;
        for (uint32_t o = 64u * t; o < span; o += 64u * LZT_THREADS) warm += lit_end[-1 - (int32_t)o];
    }
    uint32_t h_next = t < nseq ? hdr[t] : 0u;            // the next batch's header, loaded a batch ahead
    for (uint32_t s0 = 0; s0 < nseq; s0 += LZT_THREADS) {
        const svx_lzt::Seq s = svx_lzt::unpack(h_next);
        h_next = s0 + LZT_THREADS + t < nseq ? hdr[s0 + LZT_THREADS + t] : 0u;
        // (one scan for both sums: a wave's 64 sequences hold at most 64 x 513 output bytes, which fit the low half)
        const uint32_t both = svx_wave::wave_incl_scan((s.nl + s.ml) | s.nl << 16), io = both & 0xFFFFu, il = both >> 16;
        if (lane == 63) { part[wave] = io; part[LZT_WAVES + wave] = il; }
        __syncthreads();
        // lane k < LZT_WAVES of every wave takes wave k's two sums -- one round trip to LDS, not one per wave --, and their prefix
        // sums over the lanes are what lies in front of each wave and, in the last lane, the whole batch
        const uint32_t po = lane < LZT_WAVES ? part[lane] : 0u, pl = lane < LZT_WAVES ? part[LZT_WAVES + lane] : 0u;
        const uint32_t so = svx_wave::wave_incl_scan(po), sl = svx_wave::wave_incl_scan(pl);
        const int my_wave = __builtin_amdgcn_readfirstlane(wave);
        const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)so, 63), Lt = (uint32_t)__builtin_amdgcn_readlane((int)sl, 63);
        const uint32_t wo = (uint32_t)__builtin_amdgcn_readlane((int)(so - po), my_wave), wl = (uint32_t)__builtin_amdgcn_readlane((int)(sl - pl), my_wave);
        const uint32_t w = W + wo + io - (s.nl + s.ml), l = L + wl + il - s.nl;
        err = svx_lzt::batch_check(W, T, isize, L, Lt, nlit);
        // (the barrier also keeps the next batch's sums out of `part` until everybody has read this one's)
        if (__syncthreads_or(err == svx_lzt::LZ_OK && svx_lzt::seq_check(s, w) != svx_lzt::LZ_OK) && err == svx_lzt::LZ_OK) err = svx_lzt::LZ_BAD_DIST;
        if (err != svx_lzt::LZ_OK) break;                // uniform
        svx_lzt::seq_write(tab, ph, s, w, lit_end, l, LZT_PARTS);
        W += T; L += Lt;
    }
    asm volatile("" :: "v"(warm));                      // (the only use of the literals read ahead: the compiler keeps their loads)
    if (err == svx_lzt::LZ_OK && W != isize) err = svx_lzt::LZ_SHORT;
    if (err != svx_lzt::LZ_OK) { if (t == 0) status[b] = (uint32_t)err; return; }
    __syncthreads();
#if SVX_LZT_DBG & 1
    return;
#endif
    // ---- resolve
    const uint32_t nw = svx_lzt::n_words(ph, isize);
    bool done = false;
    for (uint32_t r = 0; r < svx_lzt::MAX_ROUNDS && !done; ++r) {
        bool pending = false;
#pragma unroll 1
        for (uint32_t q = t; q < nw; q += LZT_THREADS) {
            bool changed = false;
            const uint64_t v = svx_lzt::resolve_word(tab, ph, q, &changed, &pending);
            if (changed) svx_lzt::word_write(tab, q, v);
        }
        done = !__syncthreads_or(pending);
    }
    if (!done) { if (t == 0) status[b] = (uint32_t)svx_lzt::LZ_SHORT; return; }      // (cannot happen: every pointer is to a smaller position)
    // ---- emit
    const uint32_t nc = svx_lzt::n_chunks(ph, isize);
#pragma unroll 1
    for (uint32_t c = t; c < nc; c += LZT_THREADS) svx_lzt::emit_chunk(tab, ph, isize, c, out, lo);
}

}  // namespace

// (library-internal) 1 if this device can give a workgroup the table's LDS (queried once), else 0
extern "C" __attribute__((visibility("hidden"))) int svx_bgzf_lz_table_available(void)
{
    static const int ok = [] {
        int dev = 0, max_lds = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 0;
        if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) return 0;
        if ((uint32_t)max_lds < LZT_LDS) return 0;
        return hipFuncSetAttribute(reinterpret_cast<const void*>(bgzf_lz_table_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LZT_LDS) == hipSuccess ? 1 : 0;
    }();
    return ok;
}

// (library-internal) the LZ copies of a launch whose tokens kernel wrote SPLIT streams; blocks above 0xFF00 bytes get `handover`
extern "C" __attribute__((visibility("hidden"))) int svx_bgzf_lz_table(const uint8_t* streams, const void* stream_cnt, const uint64_t* d_dst_off, uint32_t n_blocks,
                                                                        uint8_t* d_out, uint32_t* d_status, uint32_t handover, void* stream)
{
    if (!svx_bgzf_lz_table_available()) return SVX_EINVAL;
    hipLaunchKernelGGL(bgzf_lz_table_kernel, dim3(n_blocks), dim3(LZT_THREADS), LZT_LDS, static_cast<hipStream_t>(stream),
                       streams, static_cast<const uint2*>(stream_cnt), d_dst_off, n_blocks, d_out, d_status, handover);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}
