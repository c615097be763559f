// svx_bamindex.hip -- where BAM records start in an inflated stream that no index describes (gfx950).
//
// The record walk of svx_bamdev.hip starts every lane at a record start the .bai linear index names.  A file without a .bai
// has one known start -- the end of its header -- and a chain of block_size fields behind it: one dependent memory round
// trip per record for whoever walks it alone.  svx_bam_find_starts finds, for every BGZF block of a range, the first record
// that starts in it -- what the walk kernels then take as their d_starts -- by speculating and verifying, as the tokens
// kernel of svx_inflate2.hip does with its Huffman segments:
//
//   speculate   one WAVE per block.  64 lanes test 64 consecutive offsets a step for "looks like a record" (looks_like_record)
//               and the wave takes the lowest that passes (a ballot): e[b].  It then walks the chain from e[b] until it leaves
//               the block: x[b] = the first chain position at or behind the block's end, succ[b] = the block x[b] lies in
//               (n_blocks: the chain ends inside the range -- on its end, or on a record the range cuts).  The block `entry`
//               lies in does not guess: its e is `entry`.
//   link        the link b -> succ[b] HOLDS iff e[succ[b]] == x[b].  jump[0][b] = succ[b] where it holds, b itself where not
//               (a stopper), and K - 1 doubling launches give jump[k][b] = the 2^k-th successor (2^K > n_blocks).
//   resolve     ONE lane.  From the entry block it descends the jump levels -- K dependent loads -- to the first stopper on the
//               true chain.  A stopper that is not the end is a broken link: a decoy was picked, or no candidate or the wrong
//               one.  The block behind it is walked from the true position x, its e / x / succ and its K jump entries (they
//               depend on the blocks behind it only, whose entries stand) are replaced, and the block becomes a marking source.
//               Every turn moves to a later block: the loop ends, after at most n_blocks turns -- a file where every guess is
//               wrong is resolved by this one lane, slowly.  Serial work: K loads + one block's records per BROKEN link.
//   mark        sources (the entry block + every re-walked block) are marked; for k = K - 1 .. 0 every marked block marks
//               jump[k][b].  A block at distance d from its source is reached through the bits of d, highest first; a stopper
//               marks itself.  Marked blocks are exactly the blocks the true chain has a start in (induction over holding links
//               from true starts).  Concurrent marks of one block store the same value: no atomics, the result is deterministic.
//   finish      d_first[b] = e[b] where marked, UINT64_MAX elsewhere (blocks a link jumps over, whatever they guessed).
//
// Correctness does not rest on looks_like_record: a wrong or missing guess costs a turn of the resolve lane, never a wrong start.
// Every read of d_raw is checked against the range's end first; nothing is read in front of d_dst_off[0].
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/svx.h"

namespace {

constexpr int WAVE = 64;
constexpr int WAVES_PER_GROUP = 4;                              // speculate: four blocks per workgroup, a wave each
constexpr int MAX_TRIES = 4;                                    // speculate: candidates whose chain is malformed before the block gives up
constexpr uint64_t NONE = ~0ull;

__device__ __forceinline__ uint32_t ld32(const uint8_t* p)    // unaligned little-endian load
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// The block an offset lies in: the LAST b with dst_off[b] <= off (blocks of no bytes in front of it are skipped); off < dst_off[n].
__device__ inline uint32_t block_of(const uint64_t* __restrict__ dst_off, uint32_t n, uint64_t off)
{
    uint32_t lo = 0, hi = n;                                    // first b in [0, n] with dst_off[b] > off
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (dst_off[mid] <= off) lo = mid + 1; else hi = mid;
    }
    return lo ? lo - 1 : 0;
}

// The fixed fields at c (c + 36 <= end checked by the caller) are those of a record: the sizes add up, the references exist.
__device__ inline bool header_plausible(const uint8_t* __restrict__ raw, uint64_t c, uint32_t n_ref, const int32_t* __restrict__ ref_len, uint32_t* bs_out)
{
    const uint32_t bs = ld32(raw + c);
    *bs_out = bs;
    if (bs < 32 || bs > 0x7FFFFFFFu) return false;
    const int32_t tid = (int32_t)ld32(raw + c + 4);
    if (tid < -1 || tid >= (int32_t)n_ref) return false;
    const int32_t pos = (int32_t)ld32(raw + c + 8);
    if (pos < -1 || (tid >= 0 && pos > ref_len[tid])) return false;
    const int32_t ntid = (int32_t)ld32(raw + c + 24);
    if (ntid < -1 || ntid >= (int32_t)n_ref) return false;
    const int32_t npos = (int32_t)ld32(raw + c + 28);
    if (npos < -1 || (ntid >= 0 && npos > ref_len[ntid])) return false;
    const uint8_t* rec = raw + c + 4;
    const uint32_t l_name = rec[8], n_cig = (uint32_t)rec[12] | (uint32_t)rec[13] << 8, l_seq = ld32(rec + 16);
    if (l_name < 1) return false;
    return 32ull + l_name + 4ull * n_cig + (l_seq + 1ull) / 2 + l_seq <= bs;
}

// A candidate passes when its header is plausible, its name ends in NUL, and the header behind it is plausible too -- where
// those bytes lie inside the range.
__device__ inline bool looks_like_record(const uint8_t* __restrict__ raw, uint64_t c, uint64_t end, uint32_t n_ref, const int32_t* __restrict__ ref_len)
{
    if (c + 36 > end) return false;
    uint32_t bs;
    if (!header_plausible(raw, c, n_ref, ref_len, &bs)) return false;
    const uint64_t name_end = c + 36 + raw[c + 12];             // (l_read_name counts the NUL)
    if (name_end > end || raw[name_end - 1] != 0) return false;
    const uint64_t q = c + 4ull + bs;
    if (q + 36 > end) return true;                              // the record behind it is not in hand: cannot tell
    uint32_t bs2;
    return header_plausible(raw, q, n_ref, ref_len, &bs2);
}

// The chain from p (a start inside the block that ends at block_end) until it leaves the block.  -> 0 and *x = the first chain
// position at or behind block_end; 1 and *x = the chain ends inside the range, on its end or on the start of a record the range
// cuts; 2 and *x = a malformed record.  The checks are those of bam_walk_count_kernel (svx_bamdev.hip).
__device__ inline int walk_block(const uint8_t* __restrict__ raw, uint64_t p, uint64_t block_end, uint64_t end, uint64_t* x)
{
    for (;;) {
        if (p >= end || p + 36 > end) { *x = p < end ? p : end; return 1; }
        const uint32_t bs = ld32(raw + p);
        const uint8_t* rec = raw + p + 4;
        const uint32_t l_name = rec[8], n_cig = (uint32_t)rec[12] | (uint32_t)rec[13] << 8, l_seq = ld32(rec + 16);
        if (bs < 32 || bs > 0x7FFFFFFFu || 32ull + l_name + 4ull * n_cig + (l_seq + 1ull) / 2 + l_seq > bs) { *x = p; return 2; }
        if (p + 4ull + bs > end) { *x = p; return 1; }
        p += 4ull + bs;
        if (p >= block_end) {
            if (p >= end) { *x = end; return 1; }
            *x = p;
            return 0;
        }
    }
}

// Workspace: e [n] u64 | x [n] u64 | succ [n] u32 | marked [n + 1] u32 | jump [K][n + 1] u32
struct Ws {
    uint64_t* e;
    uint64_t* x;
    uint32_t* succ;
    uint32_t* marked;
    uint32_t* jump;
};

__host__ __device__ inline uint32_t levels_for(uint32_t n)
{
    uint32_t k = 1;
    while ((1ull << k) <= n) ++k;                               // 2^K > n: 2^K - 1 steps reach the end from anywhere
    return k;
}

__host__ __device__ inline uint64_t pad16(uint64_t v) { return (v + 15) / 16 * 16; }

__host__ __device__ inline Ws carve(void* ws, uint32_t n)
{
    uint8_t* p = static_cast<uint8_t*>(ws);
    Ws w;
    w.e = reinterpret_cast<uint64_t*>(p);      p += pad16(8ull * n);
    w.x = reinterpret_cast<uint64_t*>(p);      p += pad16(8ull * n);
    w.succ = reinterpret_cast<uint32_t*>(p);   p += pad16(4ull * n);
    w.marked = reinterpret_cast<uint32_t*>(p); p += pad16(4ull * (n + 1ull));
    w.jump = reinterpret_cast<uint32_t*>(p);
    return w;
}

__global__ __launch_bounds__(WAVE * WAVES_PER_GROUP)
void bam_speculate_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ dst_off, uint32_t n, uint64_t entry,
                          uint32_t n_ref, const int32_t* __restrict__ ref_len, Ws w)
{
    const uint32_t b = blockIdx.x * WAVES_PER_GROUP + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (b >= n) return;                                         // (whole waves: no barrier in this kernel)
    const uint64_t lo = dst_off[b], hi = dst_off[b + 1], end = dst_off[n];
    uint64_t e = NONE, x = NONE;
    uint32_t succ = n;
    if (entry >= lo && entry < hi) {                            // the block the known start lies in: nothing to guess
        e = entry;
        const int rc = walk_block(raw, e, hi, end, &x);
        succ = rc == 0 ? block_of(dst_off, n, x) : n;
        if (rc == 2) { e = NONE; x = NONE; }                    // (the resolve lane walks it again and reports)
    } else {
        int tries = 0;
        for (uint64_t base = lo; base < hi && e == NONE && tries < MAX_TRIES; base += WAVE) {
            const uint64_t c = base + lane;
            const bool pass = c < hi && looks_like_record(raw, c, end, n_ref, ref_len);
            uint64_t mask = __ballot(pass);
            while (mask && tries < MAX_TRIES) {                 // uniform: every lane walks the lowest candidate's chain
                const uint32_t first = (uint32_t)__ffsll((unsigned long long)mask) - 1u;
                const uint64_t cand = base + first;
                const int rc = walk_block(raw, cand, hi, end, &x);
                if (rc != 2) {
                    e = cand;
                    succ = rc == 0 ? block_of(dst_off, n, x) : n;
                    break;
                }
                ++tries;                                        // a candidate whose chain is malformed is no candidate
                mask &= mask - 1;
            }
        }
        if (e == NONE) { x = NONE; succ = n; }
    }
    if (lane == 0) {
        w.e[b] = e;
        w.x[b] = x;
        w.succ[b] = succ;
        w.marked[b] = 0;
    }
}

// jump[0]: the successor where the link holds, the block itself (a stopper) where it does not; the end (n) stops too.
__global__ __launch_bounds__(256)
void bam_link_kernel(uint32_t n, Ws w)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b > n) return;
    if (b == n) { w.jump[n] = n; w.marked[n] = 0; return; }
    uint32_t j = b;
    if (w.e[b] != NONE) {
        const uint32_t s = w.succ[b];
        if (s == n || w.e[s] == w.x[b]) j = s;
    }
    w.jump[b] = j;
}

__global__ __launch_bounds__(256)
void bam_double_kernel(uint32_t n, const uint32_t* __restrict__ from, uint32_t* __restrict__ to)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b > n) return;
    to[b] = from[from[b]];
}

// ONE lane: the broken links on the true chain, one after the other (see the head of the file).
__global__ __launch_bounds__(WAVE)
void bam_resolve_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ dst_off, uint32_t n, uint64_t entry,
                        uint32_t levels, Ws w, uint64_t* __restrict__ d_exit)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t end = dst_off[n];
    if (entry < dst_off[0] || entry > end) { d_exit[0] = entry; d_exit[1] = 1; return; }
    if (entry == end) { d_exit[0] = end; d_exit[1] = 0; return; }
    const uint64_t stride = (uint64_t)n + 1;
    uint32_t cur = block_of(dst_off, n, entry);
    uint64_t at = entry;                                        // the true chain's position in front of block `cur`'s walk
    bool rewalk = w.e[cur] != entry;                            // (the entry block's own chain was malformed: walked again, reported)
    for (;;) {
        if (rewalk) {
            uint64_t x;
            const int rc = walk_block(raw, at, dst_off[cur + 1], end, &x);
            if (rc == 2) { d_exit[0] = x; d_exit[1] = 1; return; }
            const uint32_t s = rc == 0 ? block_of(dst_off, n, x) : n;
            w.e[cur] = at;
            w.x[cur] = x;
            w.succ[cur] = s;
            uint32_t j = (s == n || w.e[s] == x) ? s : cur;
            w.jump[cur] = j;
            for (uint32_t k = 1; k < levels; ++k) {             // the blocks behind `cur` keep their entries: K dependent loads
                j = w.jump[(k - 1) * stride + j];
                w.jump[k * stride + cur] = j;
            }
        }
        w.marked[cur] = 1;                                      // a marking source
        uint32_t stop = cur;
        for (uint32_t k = levels; k-- > 0;) stop = w.jump[k * stride + stop];      // 2^K - 1 > n steps: the first stopper
        if (stop == n) {
            // the chain's last block, the one whose link goes to the end: every jump that stays in front of the end is taken
            uint32_t last = cur;
            for (uint32_t k = levels; k-- > 0;) {
                const uint32_t t = w.jump[k * stride + last];
                if (t != n) last = t;
            }
            d_exit[0] = w.x[last];
            d_exit[1] = 0;
            return;
        }
        // stop -> succ[stop] does not hold: the true chain enters that block at x[stop], whatever the block guessed
        at = w.x[stop];
        cur = w.succ[stop];
        rewalk = true;
    }
}

// level k of the marking: every marked block marks its 2^k-th successor
__global__ __launch_bounds__(256)
void bam_mark_kernel(uint32_t n, const uint32_t* __restrict__ jump_k, uint32_t* __restrict__ marked)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    if (marked[b]) {
        const uint32_t t = jump_k[b];
        if (t < n && t != b) marked[t] = 1;
    }
}

__global__ __launch_bounds__(256)
void bam_first_kernel(uint32_t n, Ws w, uint64_t* __restrict__ first)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    first[b] = w.marked[b] ? w.e[b] : NONE;
}

// A lane per start: the byte offset of each of its records (the chain and the bases of bam_walk_index_kernel, svx_bamdev.hip).
__global__ __launch_bounds__(WAVE)
void bam_walk_offsets_kernel(const uint8_t* __restrict__ raw, const uint64_t* __restrict__ starts, uint32_t n_starts,
                             const uint64_t* __restrict__ base, uint64_t* __restrict__ rec_off)
{
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n_starts) return;
    uint64_t p = starts[i];
    const uint64_t end = starts[i + 1];
    uint64_t k = base[3ull * i];
    while (p < end) {                                           // (the count pass has checked the chain: it ends on `end`)
        rec_off[k++] = p;
        p += 4ull + ld32(raw + p);
    }
}

}  // namespace

extern "C" size_t svx_bam_find_starts_ws_bytes(uint32_t n_blocks)
{
    const uint64_t n = n_blocks;
    return (size_t)(2 * pad16(8 * n) + pad16(4 * n) + pad16(4 * (n + 1)) + pad16(4 * (n + 1) * (uint64_t)levels_for(n_blocks)) + 16);
}

extern "C" int svx_bam_find_starts(const uint8_t* d_raw, const uint64_t* d_dst_off, uint32_t n_blocks, uint64_t entry, uint32_t n_ref,
                                   const int32_t* d_ref_len, uint64_t* d_first, uint64_t* d_exit, void* d_ws, uint64_t ws_bytes, void* stream)
{
    if (!d_raw || !d_dst_off || !d_exit || !d_ws || n_blocks == 0 || n_blocks >= (1u << 30) || (n_ref && !d_ref_len) || !d_first) return SVX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_ws) & 15u) || ws_bytes < svx_bam_find_starts_ws_bytes(n_blocks)) return SVX_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t n = n_blocks, levels = levels_for(n);
    const Ws w = carve(d_ws, n);
    const uint64_t stride = (uint64_t)n + 1;
    const dim3 per_node((n + 1 + 255) / 256), per_block((n + 255) / 256);
    hipLaunchKernelGGL(bam_speculate_kernel, dim3((n + WAVES_PER_GROUP - 1) / WAVES_PER_GROUP), dim3(WAVE * WAVES_PER_GROUP), 0, st,
                       d_raw, d_dst_off, n, entry, n_ref, d_ref_len, w);
    hipLaunchKernelGGL(bam_link_kernel, per_node, dim3(256), 0, st, n, w);
    for (uint32_t k = 1; k < levels; ++k)
        hipLaunchKernelGGL(bam_double_kernel, per_node, dim3(256), 0, st, n, w.jump + (k - 1) * stride, w.jump + k * stride);
    hipLaunchKernelGGL(bam_resolve_kernel, dim3(1), dim3(WAVE), 0, st, d_raw, d_dst_off, n, entry, levels, w, d_exit);
    for (uint32_t k = levels; k-- > 0;)
        hipLaunchKernelGGL(bam_mark_kernel, per_block, dim3(256), 0, st, n, w.jump + k * stride, w.marked);
    hipLaunchKernelGGL(bam_first_kernel, per_block, dim3(256), 0, st, n, w, d_first);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}

extern "C" int svx_bam_walk_offsets(const uint8_t* d_raw, const uint64_t* d_starts, uint32_t n_starts, const uint64_t* d_base,
                                    uint64_t* d_rec_off, void* stream)
{
    if (n_starts == 0) return SVX_OK;
    if (!d_raw || !d_starts || !d_base || !d_rec_off) return SVX_EINVAL;
    hipLaunchKernelGGL(bam_walk_offsets_kernel, dim3((n_starts + WAVE - 1) / WAVE), dim3(WAVE), 0, static_cast<hipStream_t>(stream),
                       d_raw, d_starts, n_starts, d_base, d_rec_off);
    return hipGetLastError() == hipSuccess ? SVX_OK : SVX_ELAUNCH;
}
