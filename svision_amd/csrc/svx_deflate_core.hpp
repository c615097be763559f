// svx_deflate_core.hpp -- the phases of bgzf_deflate_kernel (svx_deflate.hip), host- and device-compilable: the CPU model
// (tools/hostwave/deflate_main.cpp) runs this very code as loops over the workgroup's threads under AddressSanitizer.
//
// One workgroup of T = 1024 threads turns one block of 0 .. 0xFF00 bytes into one BGZF member: the 18-byte header, ONE final
// DEFLATE block -- an LZ77 parse in the fixed Huffman code (BTYPE 01), or the bytes stored (BTYPE 00) whenever the fixed form
// would not be smaller --, a gap of 4 bytes for the CRC32 (svx_crc.hip fills it) and ISIZE.  The block is taken in tiles of T
// positions, thread t of a tile at position p = tile + t:
//   hash     key = the 3 bytes at p; the waves of the tile one after the other: every lane reads table[hash(key)] -- the LAST
//            position in front of its wave that hashed there --, then every lane enters its own position with an atomic max.  A
//            wave's reads come before its writes, a barrier separates the waves: what a lane reads is a function of the input
//   match    a second candidate, the nearest lane in front of p in the same wave with the same key (the table knows nothing
//            inside a wave: distance 1 lives here); the lengths of both by comparing bytes, up to 258 and the block's end; the
//            longer one wins, the nearer one at a tie.  Kept: length >= 3, distance <= 32,768, length 3 only up to distance
//            4,096 (beyond that three literals are not longer)
//   parse    greedy: the token at p is followed by the token at next[p] = p + max(1, len[p]).  The tokens of the tile are the
//            chain from `start` (where the last token of the tile in front ended): pointer jumping, next = next[next], marks
//            positions 2^r links apart in round r -- 10 rounds
//   bits     every token's code (Huffman codes most significant bit first, extra bits least significant bit first, packed
//            into one value of <= 31 bits); a prefix sum of the lengths; atomic OR into a staging area of whole words; the
//            tile's whole bytes go to the member, the last partial byte opens the next tile's staging area
// Everything a thread reads was written in front of a barrier, or by an atomic whose result does not depend on the order
// (max, or).  The one exception is `mark` in the parse rounds: a thread reads mark[t] while another may store mark[t] = 1 in
// the same round, neither access atomic.  The only value ever stored is 1, a mark only lands on a position of the chain, and
// after round r the chain's first 2^(r+1) positions are marked whichever way each read fell (a mark seen early only marks a
// chain position sooner), so after the last round the marks are the chain and nothing else in every order.
// Hence the member is a pure function of the block's bytes.  Fixed bytes are written only below the stored form's
// size, so a block that turns out to be stored never wrote past byte 18 + n + 5 of its slot.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SVX_DFL_HD __host__ __device__ __forceinline__
#else
#define SVX_DFL_HD inline
#endif

namespace svx_dfl {

constexpr uint32_t T = 1024, WAVE = 64, WAVES = T / WAVE;
constexpr uint32_t MAX_IN = 0xFF00;                  // the largest block
constexpr uint32_t TABLE_BITS = 14, TABLE_ENTRIES = 1u << TABLE_BITS;
constexpr uint32_t MIN_MATCH = 3, MAX_MATCH = 258, MAX_DIST = 32768, MAX_DIST_LEN3 = 4096;
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;
constexpr uint32_t STAGE_WORDS = T;                  // 7 carried bits + T tokens of <= 31 bits < 32 T bits
constexpr uint32_t HEADER = 18, FOOTER = 8, STORED_EXTRA = 5;
constexpr uint32_t SLOT = 65536;                     // a member's slot in the encoder's output; the largest member is 0xFF00 + 31 bytes

// the workgroup's LDS (the host model: heap blocks of exactly these sizes)
struct Ctx {
    uint8_t* in;          // [n]                 the block
    uint32_t* table;      // [TABLE_ENTRIES]     hash -> last position + 1, 0 = none
    uint32_t* keys;       // [T]                 the tile's keys
    uint32_t* cand;       // [T]                 the table's candidate + 1; later the token's bits
    uint16_t* mlen;       // [T]                 match length, 0 = literal
    uint16_t* mdist;      // [T]                 distance - 1
    uint16_t* nxt_a;      // [T]                 the chain's links, two copies that take turns
    uint16_t* nxt_b;      // [T]
    uint8_t* mark;        // [T]                 1: a token starts here
    uint32_t* tokoff;     // [T]                 token bit lengths -> their exclusive prefix sum
    uint32_t* stage;      // [STAGE_WORDS]       the tile's bits
    uint32_t* s;          // [4]                 uniform state: S_START, S_BITS, S_LEFT, S_FIXED
};
enum { S_START = 0, S_BITS = 1, S_LEFT = 2, S_FIXED = 3 };
constexpr uint32_t LDS_BYTES = (MAX_IN + 3u) / 4u * 4u + 4u * TABLE_ENTRIES + 4u * T * 4u + 2u * T * 4u + T + 16u;

// carve the context out of one 16-byte aligned block of LDS_BYTES bytes
SVX_DFL_HD Ctx carve(uint8_t* lds)
{
    Ctx c;
    uint8_t* q = lds;
    c.table = reinterpret_cast<uint32_t*>(q); q += 4u * TABLE_ENTRIES;
    c.keys = reinterpret_cast<uint32_t*>(q); q += 4u * T;
    c.cand = reinterpret_cast<uint32_t*>(q); q += 4u * T;
    c.tokoff = reinterpret_cast<uint32_t*>(q); q += 4u * T;
    c.stage = reinterpret_cast<uint32_t*>(q); q += 4u * STAGE_WORDS;
    c.s = reinterpret_cast<uint32_t*>(q); q += 16u;
    c.mlen = reinterpret_cast<uint16_t*>(q); q += 2u * T;
    c.mdist = reinterpret_cast<uint16_t*>(q); q += 2u * T;
    c.nxt_a = reinterpret_cast<uint16_t*>(q); q += 2u * T;
    c.nxt_b = reinterpret_cast<uint16_t*>(q); q += 2u * T;
    c.mark = q; q += T;
    c.in = q;
    return c;
}

SVX_DFL_HD uint32_t key3(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16; }
SVX_DFL_HD uint32_t hash3(uint32_t key) { return (key * 2654435761u) >> (32u - TABLE_BITS); }
SVX_DFL_HD uint32_t bit_length(uint32_t v) { return v ? 32u - (uint32_t)__builtin_clz(v) : 0u; }
SVX_DFL_HD uint32_t rev_bits(uint32_t v, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1u - i);
    return r;
}

// bytes [c, c + l) == bytes [p, p + l), c < p, the longest l <= maxl (p + maxl <= n: no read behind the block)
SVX_DFL_HD uint32_t match_len(const uint8_t* in, uint32_t c, uint32_t p, uint32_t maxl)
{
    uint32_t l = 0;
    while (l < maxl && in[c + l] == in[p + l]) ++l;
    return l;
}

// a symbol of the literal/length alphabet in the fixed code, bit-reversed for the LSB-first stream -> value, *n its bits
SVX_DFL_HD uint32_t fixed_code(uint32_t sym, uint32_t* n)
{
    if (sym < 144u) { *n = 8; return rev_bits(0x30u + sym, 8); }
    if (sym < 256u) { *n = 9; return rev_bits(0x190u + (sym - 144u), 9); }
    if (sym < 280u) { *n = 7; return rev_bits(sym - 256u, 7); }
    *n = 8; return rev_bits(0xC0u + (sym - 280u), 8);
}

// the token at a position: literal `byte` (len 0) or the match (len, dist) -> its bits, first bit lowest; *n <= 31
SVX_DFL_HD uint32_t token_bits(uint32_t byte, uint32_t len, uint32_t dist, uint32_t* n)
{
    if (len == 0) return fixed_code(byte, n);
    uint32_t sym, le = 0, lx = 0;                    // length symbol, extra bits and their value
    const uint32_t l = len - 3u;
    if (len == 258u) sym = 285u;
    else if (l < 8u) sym = 257u + l;
    else { le = bit_length(l) - 3u; sym = 257u + 4u * (le + 1u) + ((l >> le) & 3u); lx = l & ((1u << le) - 1u); }
    uint32_t nb, v = fixed_code(sym, &nb);
    v |= lx << nb; nb += le;
    const uint32_t dd = dist - 1u;
    uint32_t dsym = dd, de = 0, dx = 0;
    if (dd >= 4u) { de = bit_length(dd) - 2u; dsym = 2u * de + 2u + ((dd >> de) & 1u); dx = dd & ((1u << de) - 1u); }
    v |= rev_bits(dsym, 5) << nb; nb += 5u;
    v |= dx << nb; nb += de;
    *n = nb;
    return v;
}

// the 18 bytes in front of every member's payload; bytes 16, 17 = the member's length - 1
SVX_DFL_HD void write_header(uint8_t* m, uint32_t member_len)
{
    const uint8_t h[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    for (int i = 0; i < 16; ++i) m[i] = h[i];
    m[16] = (uint8_t)((member_len - 1u) & 255u); m[17] = (uint8_t)((member_len - 1u) >> 8);
}

// One block.  E: each(f) runs f(t) for every thread t of the workgroup; barrier(); wave_sync() orders the accesses of one
// wave's lanes (the device: lockstep, the host model: a loop's end); atomic_max / atomic_or on LDS words; scan(a, &total):
// a[T] -> its exclusive prefix sum, in place, between barriers of its own.  src [n] -> slot [18 + min(n + 5, fixed) + 8],
// *member_len, *stored (1: BTYPE 00).  The CRC32's 4 bytes at member_len - 8 are left for the caller.
template <class E>
SVX_DFL_HD void encode_block(E& ex, const Ctx& c, const uint8_t* src, uint32_t n, uint8_t* slot, uint32_t* member_len, uint32_t* stored)
{
    const uint32_t cap = n + STORED_EXTRA;           // fixed bytes at and beyond this index are never written: the block is stored then
    ex.each([&](uint32_t t) {
        for (uint32_t i = t; i < TABLE_ENTRIES; i += T) c.table[i] = 0;
        for (uint32_t i = t; i < n; i += T) c.in[i] = src[i];
        for (uint32_t i = t; i < STAGE_WORDS; i += T) c.stage[i] = 0;
    });
    ex.barrier();
    ex.each([&](uint32_t t) {
        if (t == 0) { c.s[S_START] = 0; c.s[S_BITS] = 3; c.stage[0] = 3; }       // BFINAL 1, BTYPE 01 (least significant bit first: 1, 1, 0)
    });
    ex.barrier();
    for (uint32_t tile = 0; tile < n; tile += T) {
        const uint32_t cnt = n - tile < T ? n - tile : T;
        // ---- hash
        ex.each([&](uint32_t t) {
            const uint32_t p = tile + t;
            c.keys[t] = p + MIN_MATCH <= n ? key3(c.in + p) : NO_KEY;
            c.cand[t] = 0;
        });
        for (uint32_t w = 0; w * WAVE < cnt; ++w) {
            ex.each([&](uint32_t t) { if (t / WAVE == w && c.keys[t] != NO_KEY) c.cand[t] = c.table[hash3(c.keys[t])]; });
            ex.wave_sync();
            ex.each([&](uint32_t t) { if (t / WAVE == w && c.keys[t] != NO_KEY) ex.atomic_max(&c.table[hash3(c.keys[t])], tile + t + 1u); });
            ex.barrier();
        }
        // ---- match
        ex.each([&](uint32_t t) {
            const uint32_t p = tile + t, k = c.keys[t];
            uint32_t len = 0, dist = 0;
            if (k != NO_KEY) {
                const uint32_t maxl = n - p < MAX_MATCH ? n - p : MAX_MATCH;
                if (c.cand[t] != 0 && p - (c.cand[t] - 1u) <= MAX_DIST) { dist = p - (c.cand[t] - 1u); len = match_len(c.in, p - dist, p, maxl); }
                for (uint32_t d = 1; d <= t % WAVE; ++d)
                    if (c.keys[t - d] == k) {
                        const uint32_t l2 = match_len(c.in, p - d, p, maxl);
                        if (l2 >= len) { len = l2; dist = d; }
                        break;
                    }
                if (len < MIN_MATCH || (len == MIN_MATCH && dist > MAX_DIST_LEN3)) len = 0;
            }
            c.mlen[t] = (uint16_t)len;
            c.mdist[t] = (uint16_t)(len ? dist - 1u : 0u);
            const uint32_t nx = t + (len ? len : 1u);
            c.nxt_a[t] = (uint16_t)(t < cnt && nx < cnt ? nx : T);
            c.mark[t] = 0;
        });
        ex.barrier();
        // ---- parse
        ex.each([&](uint32_t t) { if (t == 0 && c.s[S_START] - tile < cnt) c.mark[c.s[S_START] - tile] = 1; });
        ex.barrier();
        uint16_t *a = c.nxt_a, *b = c.nxt_b;
        for (uint32_t r = 0; (1u << r) < cnt; ++r) {
            ex.each([&](uint32_t t) {
                const uint32_t nx = a[t];
                if (nx < T) { if (c.mark[t]) c.mark[nx] = 1; b[t] = a[nx]; } else b[t] = (uint16_t)T;
            });
            ex.barrier();
            uint16_t* const sw = a; a = b; b = sw;
        }
        // ---- bits
        ex.each([&](uint32_t t) {
            uint32_t nb = 0, v = 0;
            if (t < cnt && c.mark[t]) {
                const uint32_t len = c.mlen[t];
                v = token_bits(c.in[tile + t], len, (uint32_t)c.mdist[t] + 1u, &nb);
                if (t + (len ? len : 1u) >= cnt) c.s[S_START] = tile + t + (len ? len : 1u);     // the chain's last token of the tile: one thread
            }
            c.cand[t] = v;
            c.tokoff[t] = nb;
        });
        uint32_t total = 0;
        ex.scan(c.tokoff, &total);
        ex.each([&](uint32_t t) {
            if (t < cnt && c.mark[t]) {
                const uint32_t o = (c.s[S_BITS] & 7u) + c.tokoff[t];
                const uint64_t v = (uint64_t)c.cand[t] << (o & 31u);
                ex.atomic_or(&c.stage[o >> 5], (uint32_t)v);
                if ((uint32_t)(v >> 32)) ex.atomic_or(&c.stage[(o >> 5) + 1u], (uint32_t)(v >> 32));
            }
        });
        ex.barrier();
        // ---- the tile's whole bytes to the member
        ex.each([&](uint32_t t) {
            const uint32_t bits = c.s[S_BITS], base = bits >> 3, nfull = ((bits & 7u) + total) >> 3;
            for (uint32_t k = t; k < nfull; k += T)
                if (base + k < cap) slot[HEADER + base + k] = (uint8_t)(c.stage[k >> 2] >> (8u * (k & 3u)));
            if (t == 0) c.s[S_LEFT] = (c.stage[nfull >> 2] >> (8u * (nfull & 3u))) & 255u;
        });
        ex.barrier();
        ex.each([&](uint32_t t) {
            for (uint32_t i = t; i < STAGE_WORDS; i += T) c.stage[i] = i == 0 ? c.s[S_LEFT] : 0u;
        });
        ex.barrier();
        ex.each([&](uint32_t t) { if (t == 0) c.s[S_BITS] += total; });
        ex.barrier();
    }
    // ---- end of block (7 zero bits), the choice, header and ISIZE
    ex.each([&](uint32_t t) {
        if (t == 0) {
            const uint32_t bits = c.s[S_BITS], base = bits >> 3, fixed = (bits + 7u + 7u) >> 3;
            for (uint32_t k = base; k < fixed; ++k)
                if (k < cap) slot[HEADER + k] = (uint8_t)(k == base ? c.stage[0] & 255u : 0u);
            c.s[S_FIXED] = fixed;
        }
    });
    ex.barrier();
    ex.each([&](uint32_t t) {
        const uint32_t fixed = c.s[S_FIXED];
        const bool st = fixed >= cap;
        const uint32_t payload = st ? cap : fixed, len = HEADER + payload + FOOTER;
        if (st) {
            for (uint32_t i = t; i < n; i += T) slot[HEADER + STORED_EXTRA + i] = c.in[i];
            if (t == 0) {
                uint8_t* q = slot + HEADER;
                q[0] = 1; q[1] = (uint8_t)(n & 255u); q[2] = (uint8_t)(n >> 8); q[3] = (uint8_t)(~n & 255u); q[4] = (uint8_t)((~n >> 8) & 255u);
            }
        }
        if (t == 0) {
            write_header(slot, len);
            uint8_t* q = slot + HEADER + payload + 4u;
            q[0] = (uint8_t)(n & 255u); q[1] = (uint8_t)(n >> 8); q[2] = 0; q[3] = 0;
            *member_len = len;
            *stored = st ? 1u : 0u;
        }
    });
}

}  // namespace svx_dfl
