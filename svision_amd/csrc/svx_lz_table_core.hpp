// svx_lz_table_core.hpp -- the phases of bgzf_lz_table_kernel (svx_lz_table.hip), host- and device-compilable: the CPU model
// (tools/hostwave/lz_table_main.cpp) runs this very code against zlib under AddressSanitizer.
//
// Every byte of a BGZF block's output is a literal or a copy of the byte `distance` positions in front of it -- a strictly
// smaller position, overlapping matches included.  So the block is a forest of pointers src[p] = p - distance with the literals
// as roots, and pointer jumping, src[p] = src[src[p]], halves every chain per round: chains are at most 65,279 long, 17 rounds
// resolve any block, and there is no order between sequences and no case for overlapping matches.
//
// The table: one u16 entry per output byte.  htslib and this project's writer never put more than 0xFF00 bytes into a block,
// so the values 0xFF00 .. 0xFFFF are free to carry the 256 byte values:
//   entry <  0xFF00  a pointer: the POSITION (in the block) of the byte this one copies
//   entry >= 0xFF00  a resolved byte, entry & 0xFF
// Entry of position p lives at index ph + p, ph = the output's address mod 16: the 16 entries at an index that is a multiple of 16
// are then one aligned 16-byte chunk of the output.  The (< 16) entries in front of position 0 and behind the last one, up to
// the next multiple of 16, are set to "resolved": the resolve and emit steps work on whole groups of 4 and 16 entries.
//
// Input: the SPLIT sequence stream of bgzf_tokens_kernel<true> (svx_inflate2.hip) -- u32 headers [literals:8 | match length:9 |
// distance - 1:15] as an array, literal j of the block at lit_end[-1 - j].
//
// Every index into the table is a loop index below the block's own (rounded) size or ph + a value just tested < 0xFF00: no
// input can index outside TABLE_ENTRIES entries.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SVX_LZT_HD __host__ __device__ __forceinline__
#define SVX_LZT_ROLLED _Pragma("unroll 1")          // (unrolled, the build loops cost the kernel 30 registers)
#else
#define SVX_LZT_HD inline
#define SVX_LZT_ROLLED
#endif

namespace svx_lzt {

constexpr uint32_t MAX_OUT = 0xFF00;                 // the largest block the table takes; entries >= MAX_OUT are resolved bytes
constexpr uint32_t TABLE_ENTRIES = MAX_OUT + 16;     // + the output phase, rounded up to a chunk
constexpr uint32_t TABLE_BYTES = 2 * TABLE_ENTRIES;
constexpr uint32_t MAX_ROUNDS = 17;                  // 1 + ceil(log2(65,279)): the resolve loop's hard cap
constexpr uint64_t ALL_RESOLVED = 0xFF00FF00FF00FF00ull;
enum { LZ_OK = 0, LZ_OUT_OVERRUN = 5, LZ_SHORT = 7, LZ_BAD_DIST = 8 };      // (the codes of svx_lz_core.hpp)

struct Seq { uint32_t nl, ml, d; };
SVX_LZT_HD Seq unpack(uint32_t h) { return Seq{h & 255u, (h >> 8) & 511u, (h >> 17) + 1u}; }

SVX_LZT_HD uint32_t round16(uint32_t v) { return (v + 15u) & ~15u; }
SVX_LZT_HD uint32_t n_words(uint32_t ph, uint32_t isize) { return round16(ph + isize) / 4u; }       // groups of 4 entries
SVX_LZT_HD uint32_t n_chunks(uint32_t ph, uint32_t isize) { return round16(ph + isize) / 16u; }     // groups of 16 entries

// where block b's sequence stream lies in the workspace of svx_bgzf_inflate_fast: 1.5 x the inflated bytes in front of it + 1 KB per block
SVX_LZT_HD uint64_t slot_at(uint64_t d, uint32_t b) { return d + (d >> 1) + 1024ull * b; }      // d = the inflated bytes in front of block b
SVX_LZT_HD uint64_t slot_base(const uint64_t* dst_off, uint32_t b) { return slot_at(dst_off[b] - dst_off[0], b); }

// ---- build
// thread t < 32 of the block: the entries in front of position 0 (t < 16) and behind position isize - 1 (t >= 16)
SVX_LZT_HD void pad_write(uint16_t* tab, uint32_t ph, uint32_t isize, uint32_t t)
{
    if (t < 16u) { if (t < ph) tab[t] = (uint16_t)MAX_OUT; }
    else { const uint32_t e = ph + isize + (t - 16u); if (e < round16(ph + isize)) tab[e] = (uint16_t)MAX_OUT; }
}

// a batch of sequences that starts at position W, behind L literals, and holds T output and Lt literal bytes in all
SVX_LZT_HD int batch_check(uint32_t W, uint32_t T, uint32_t isize, uint32_t L, uint32_t Lt, uint32_t nlit)
{
    return (W + T > isize || L + Lt > nlit) ? LZ_OUT_OVERRUN : LZ_OK;
}

// one sequence whose first byte is position w: the match may reach back to the block's first byte, not further
SVX_LZT_HD int seq_check(Seq s, uint32_t w) { return (s.ml && s.d > w + s.nl) ? LZ_BAD_DIST : LZ_OK; }

// one checked sequence at position w, its first literal the block's l-th: w + nl + ml <= isize <= MAX_OUT, l + nl <= nlit.
// `parts`: measurement builds only (SVX_LZT_DBG: 1 = the literal part, 2 = the match part; both everywhere else)
SVX_LZT_HD void seq_write(uint16_t* tab, uint32_t ph, Seq s, uint32_t w, const uint8_t* lit_end, uint32_t l, uint32_t parts = 3u)
{
    uint16_t* e = tab + ph + w;
    const uint8_t* q = lit_end - 1 - l;
    if (parts & 1u) {
        SVX_LZT_ROLLED
        for (uint32_t k = 0; k < s.nl; ++k) e[k] = (uint16_t)(MAX_OUT | q[-(int32_t)k]);
    }
    e += s.nl;
    const uint32_t from = w + s.nl - s.d;
    if (parts & 2u) {
        SVX_LZT_ROLLED
        for (uint32_t k = 0; k < s.ml; ++k) e[k] = (uint16_t)(from + k);
    }
}

// ---- resolve: one step of one thread = the 4 entries of word q (8-byte aligned; only this thread ever writes them).  Reads the
// word and, for every pointer in it, the pointer's target; -> the word to write back (*changed: it differs), *pending: a pointer
// is left in it.  A target read while its owner updates it is the old pointer or the new one or the value: all of them
// ancestors of this entry, so the result is the same whatever the timing.
SVX_LZT_HD uint64_t resolve_word(const uint16_t* tab, uint32_t ph, uint32_t q, bool* changed, bool* pending)
{
    tab = static_cast<const uint16_t*>(__builtin_assume_aligned(tab, 16));
    uint64_t cur;
    memcpy(&cur, tab + 4u * q, 8);
    if ((cur & ALL_RESOLVED) == ALL_RESOLVED) return cur;       // (a pointer's high byte is below 0xFF)
    uint64_t nxt = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (uint32_t j = 0; j < 4; ++j) {
        uint32_t a = (uint32_t)(cur >> (16u * j)) & 0xFFFFu;
        if (a < MAX_OUT) {
            a = tab[ph + a];
            if (a < MAX_OUT) *pending = true;
        }
        nxt |= (uint64_t)a << (16u * j);
    }
    *changed = nxt != cur;
    return nxt;
}

SVX_LZT_HD void word_write(uint16_t* tab, uint32_t q, uint64_t v) { memcpy(static_cast<uint16_t*>(__builtin_assume_aligned(tab, 16)) + 4u * q, &v, 8); }

// 16 entries from the table / 16 bytes to the output, both 16-byte aligned.  (On the device as vector accesses by name: from a
// memcpy the compiler derives sixteen one-byte LDS reads and a store in three pieces.)
SVX_LZT_HD void load_chunk(uint32_t* e, const uint16_t* from)
{
#ifdef __HIP_DEVICE_COMPILE__
    const uint4 a = reinterpret_cast<const uint4*>(from)[0], b = reinterpret_cast<const uint4*>(from)[1];
    e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w; e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
#else
    memcpy(e, __builtin_assume_aligned(from, 16), 32);
#endif
}
SVX_LZT_HD void store_chunk(uint8_t* to, const uint32_t* v)
{
#ifdef __HIP_DEVICE_COMPILE__
    *reinterpret_cast<uint4*>(to) = make_uint4(v[0], v[1], v[2], v[3]);
#else
    memcpy(__builtin_assume_aligned(to, 16), v, 16);
#endif
}

// ---- emit: chunk c = the entries [16 c, 16 c + 16) = the output bytes out[lo - ph + 16 c ...): one aligned 16-byte store where
// the whole chunk is this block's, byte-wise at the block's two ends (the neighbouring bytes belong to other blocks).  `out` is
// 16-byte aligned.
SVX_LZT_HD void emit_chunk(const uint16_t* tab, uint32_t ph, uint32_t isize, uint32_t c, uint8_t* out, uint64_t lo)
{
    uint32_t e[8], v[4];                             // 16 entries -> their low bytes
    load_chunk(e, tab + 16u * c);
    for (uint32_t i = 0; i < 4; ++i)
        v[i] = (e[2 * i] & 0xFFu) | ((e[2 * i] >> 8) & 0xFF00u) | ((e[2 * i + 1] & 0xFFu) << 16) | ((e[2 * i + 1] << 8) & 0xFF000000u);
    const uint32_t first = 16u * c;                  // index of the chunk's first entry; its position is first - ph
    if (first >= ph && first + 16u <= ph + isize) store_chunk(out + (lo - ph + first), v);
    else
        for (uint32_t i = 0; i < 16; ++i)
            if (first + i >= ph && first + i < ph + isize) out[lo - ph + first + i] = (uint8_t)(v[i >> 2] >> (8u * (i & 3u)));
}

}  // namespace svx_lzt
