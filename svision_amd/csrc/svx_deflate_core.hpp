// svx_deflate_core.hpp -- the phases of bgzf_deflate_kernel and bgzf_deflate_dyn_kernel (svx_deflate.hip), host- and device-compilable:
// the CPU models (tools/hostwave/deflate_main.cpp, deflate_dyn_main.cpp) run this very code as loops over the workgroup's threads under
// AddressSanitizer.  First the fixed encoder and the phases both share (load_block, parse_tile, close_member); the dynamic encoder and
// what it adds stand behind encode_block.
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

// a match length 3 .. 258 -> its symbol 257 .. 285, *le its extra bits and *lx their value
SVX_DFL_HD uint32_t len_symbol(uint32_t len, uint32_t* le, uint32_t* lx)
{
    const uint32_t l = len - 3u;
    *le = 0; *lx = 0;
    if (len == 258u) return 285u;
    if (l < 8u) return 257u + l;
    const uint32_t e = bit_length(l) - 3u;
    *le = e; *lx = l & ((1u << e) - 1u);
    return 257u + 4u * (e + 1u) + ((l >> e) & 3u);
}

// a distance 1 .. 32,768 -> its symbol 0 .. 29, *de its extra bits and *dx their value
SVX_DFL_HD uint32_t dist_symbol(uint32_t dist, uint32_t* de, uint32_t* dx)
{
    const uint32_t dd = dist - 1u;
    *de = 0; *dx = 0;
    if (dd < 4u) return dd;
    const uint32_t e = bit_length(dd) - 2u;
    *de = e; *dx = dd & ((1u << e) - 1u);
    return 2u * e + 2u + ((dd >> e) & 1u);
}

// the token at a position: literal `byte` (len 0) or the match (len, dist) -> its bits in the FIXED code, first bit lowest; *n <= 31
SVX_DFL_HD uint32_t token_bits(uint32_t byte, uint32_t len, uint32_t dist, uint32_t* n)
{
    if (len == 0) return fixed_code(byte, n);
    uint32_t le, lx, de, dx;
    const uint32_t sym = len_symbol(len, &le, &lx), dsym = dist_symbol(dist, &de, &dx);
    uint32_t nb, v = fixed_code(sym, &nb);
    v |= lx << nb; nb += le;
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

// E, the workgroup as the phases see it: each(f) runs f(t) for every thread t of the workgroup; barrier(); wave_sync() orders the
// accesses of one wave's lanes (the device: lockstep, the host model: a loop's end); atomic_max / atomic_or (the dynamic encoder:
// atomic_add too, and tick(k), which may read a clock at the k-th of its four phase boundaries) on LDS words; scan(a, &total): a[T] -> its exclusive prefix sum, in place, between barriers of its own.

// the block into LDS, table and staging area empty (no barrier behind it)
template <class E>
SVX_DFL_HD void load_block(E& ex, const Ctx& c, const uint8_t* src, uint32_t n)
{
    ex.each([&](uint32_t t) {
        for (uint32_t i = t; i < TABLE_ENTRIES; i += T) c.table[i] = 0;
        for (uint32_t i = t; i < n; i += T) c.in[i] = src[i];
        for (uint32_t i = t; i < STAGE_WORDS; i += T) c.stage[i] = 0;
    });
}

// hash, match and parse of the tile's cnt positions: mlen / mdist hold every position's match, mark the tokens of the chain from
// s[S_START]
template <class E>
SVX_DFL_HD void parse_tile(E& ex, const Ctx& c, uint32_t n, uint32_t tile, uint32_t cnt)
{
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
}

// the member around a payload that is decided: the bytes stored (st) or `coded` bytes already in the slot; header, ISIZE, *member_len
template <class E>
SVX_DFL_HD void close_member(E& ex, const Ctx& c, uint32_t n, uint8_t* slot, bool st, uint32_t coded, uint32_t* member_len)
{
    ex.each([&](uint32_t t) {
        const uint32_t payload = st ? n + STORED_EXTRA : coded, len = HEADER + payload + FOOTER;
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
        }
    });
}

// One block in the fixed code or stored.  src [n] -> slot [18 + min(n + 5, fixed) + 8], *member_len, *stored (1: BTYPE 00).  The
// CRC32's 4 bytes at member_len - 8 are left for the caller.
template <class E>
SVX_DFL_HD void encode_block(E& ex, const Ctx& c, const uint8_t* src, uint32_t n, uint8_t* slot, uint32_t* member_len, uint32_t* stored)
{
    const uint32_t cap = n + STORED_EXTRA;           // fixed bytes at and beyond this index are never written: the block is stored then
    load_block(ex, c, src, n);
    ex.barrier();
    ex.each([&](uint32_t t) {
        if (t == 0) { c.s[S_START] = 0; c.s[S_BITS] = 3; c.stage[0] = 3; }       // BFINAL 1, BTYPE 01 (least significant bit first: 1, 1, 0)
    });
    ex.barrier();
    for (uint32_t tile = 0; tile < n; tile += T) {
        const uint32_t cnt = n - tile < T ? n - tile : T;
        parse_tile(ex, c, n, tile, cnt);
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
    const uint32_t fixed = c.s[S_FIXED];
    close_member(ex, c, n, slot, fixed >= cap, fixed, member_len);
    ex.each([&](uint32_t t) { if (t == 0) *stored = fixed >= cap ? 1u : 0u; });
}

// ================================================================================================================================
// The dynamic encoder (bgzf_deflate_dyn_kernel): the same parse, ONE final block in the smallest of three forms -- stored, the fixed
// code, or Huffman codes built from the block's own tokens (BTYPE 10).
//   record   per tile, in place of the bits phase: every token of the chain goes to the caller's workspace -- a match as 23 bits
//            (length - 3, distance - 1) in the 3 bytes of its first 3 positions, a literal not at all (the block stays in LDS), and
//            one bit a position that says where a token starts; a token is a match where the position behind it starts none -- and
//            into two histograms in LDS, literal/length and distance: integer atomic adds
//   codes    per alphabet (build_code): the used symbols ranked by (count, symbol), every thread its own rank; Huffman's merge over
//            the ranked leaves with two queues, one lane, a leaf in front of a node of equal weight; every leaf's depth by walking up;
//            the counts per length, depths above the limit counted at the limit, and zlib's repair until the Kraft sum is 1 again (each
//            step: one leaf of the longest length below the limit moves a level down and takes a leaf of the limit's length as its
//            sibling); the lengths handed out by rank, longest first.  An alphabet with fewer than two used symbols gets zlib's
//            stand-ins (symbols 0 and 1, or the one next to a lone low symbol) at count 1: every code is complete.  Then the two codes'
//            lengths as zlib's run-length sequence (16, 17, 18; the two alphabets separately), HLIT and HDIST trimmed, and the code
//            for that sequence the same way, at most 7 bits, HCLEN trimmed
//   choice   the three sizes from the histograms and lengths, before a bit is written: stored at a tie, then fixed, then dynamic
//   emit     the code tables hold the fixed or the built lengths; canonical codes from them; the header sequence and then the recorded
//            tokens tile by tile: a token's two halves (length code + extra bits <= 20, distance code + extra bits <= 28), a prefix sum,
//            atomic OR into a staging area for 48 bits a token in the LDS the hash table has left
// Ties are broken by symbol index everywhere and the sums do not depend on the order of the adds, so the member stays a pure function
// of the block's bytes; where stored or fixed wins it is encode_block's member, byte for byte.
constexpr uint32_t NLIT = 288, NDIST = 32, NCL = 19, NCL_ROOM = 32;   // alphabets (the fixed code counts 288 and 32 symbols)
constexpr uint32_t USED_LIT = 286, USED_DIST = 30, EOB = 256;
constexpr uint32_t CODE_BITS = 15, CL_BITS = 7;
constexpr uint32_t SEQ_ROOM = NLIT + NDIST;                      // the code-length sequence: at most 286 + 30 entries
constexpr uint32_t STAGE2_WORDS = (7u + 48u * T + 31u) / 32u + 1u;     // 7 carried bits + T tokens of <= 48 bits
constexpr uint32_t WS_MARK_WORDS = (MAX_IN + 31u) / 32u;
constexpr uint32_t WS_BLOCK = MAX_IN + 4u * WS_MARK_WORDS;       // workspace bytes a block: token bytes, then the mark words
constexpr uint32_t HIST_BYTES = 4u * (NLIT + NDIST);
constexpr uint32_t DYN_LDS_BYTES = LDS_BYTES + HIST_BYTES;
enum { ST_USED = 16, ST_TOP = 17, ST_WORDS = 32 };               // Huff::st: [1 .. 15] symbols per length
enum { D_DYN = 0, D_FIX = 1, D_FORM = 2, D_PAYLOAD = 3, D_HLIT = 4, D_HDIST = 5, D_HCLEN = 6, D_SEQ = 7, D_END = 8, D_WORDS = 16 };
enum { FORM_STORED = 0, FORM_FIXED = 1, FORM_DYNAMIC = 2 };

struct Huff {             // one alphabet of n symbols, code lengths <= maxbits
    uint32_t* w;          // [n]       weights: the counts, stand-ins at 1
    uint32_t* sw;         // [n]       the used symbols' weights by rank
    uint32_t* nfreq;      // [n]       the merged nodes' weights
    uint16_t* order;      // [n]       rank -> symbol
    uint16_t* parent;     // [2 n]     leaf (by rank) or node n + j -> node
    uint8_t* len;         // [n]       code lengths, 0 = unused
    uint16_t* code;       // [n]       the codes, bit-reversed
    uint32_t* st;         // [ST_WORDS]
    uint32_t n, maxbits;
};

struct DynCtx {
    uint32_t* hist_lit;   // [NLIT]    LDS of its own: alive during the parse
    uint32_t* hist_dist;  // [NDIST]
    Huff lit, dist, cl;   // everything from here on lies where the hash table was
    uint8_t* seq_sym;     // [SEQ_ROOM] the code-length sequence: symbols 0 .. 18
    uint8_t* seq_ext;     // [SEQ_ROOM] and the extra bits' value of 16, 17, 18
    uint32_t* ds;         // [D_WORDS]
    uint32_t* stage2;     // [STAGE2_WORDS]
    uint8_t* ws_tok;      // [n]       workspace (global memory): a match's 23 bits at its first 3 positions
    uint32_t* ws_mark;    // [(n + 31) / 32]  bit p: a token starts at position p
};

SVX_DFL_HD uint8_t* carve_huff(Huff* h, uint8_t* q, uint32_t n, uint32_t maxbits)
{
    h->n = n; h->maxbits = maxbits;
    h->w = reinterpret_cast<uint32_t*>(q); q += 4u * n;
    h->sw = reinterpret_cast<uint32_t*>(q); q += 4u * n;
    h->nfreq = reinterpret_cast<uint32_t*>(q); q += 4u * n;
    h->st = reinterpret_cast<uint32_t*>(q); q += 4u * ST_WORDS;
    h->order = reinterpret_cast<uint16_t*>(q); q += 2u * n;
    h->parent = reinterpret_cast<uint16_t*>(q); q += 4u * n;
    h->code = reinterpret_cast<uint16_t*>(q); q += 2u * n;
    h->len = q; q += n;
    return q;
}
constexpr uint32_t HUFF_BYTES(uint32_t n) { return 21u * n + 4u * ST_WORDS; }
constexpr uint32_t DYN_SCRATCH = HUFF_BYTES(NLIT) + 2u * HUFF_BYTES(NDIST) + 2u * SEQ_ROOM + 4u * D_WORDS + 4u * STAGE2_WORDS;
static_assert(DYN_SCRATCH <= 4u * TABLE_ENTRIES, "the code construction and the staging area live in the hash table's LDS");
static_assert(NCL_ROOM == NDIST && HUFF_BYTES(NLIT) % 4u == 0 && HUFF_BYTES(NDIST) % 4u == 0, "carve_dyn keeps its words aligned");

// the dynamic encoder's context out of one 16-byte aligned block of DYN_LDS_BYTES bytes; c = carve(lds) of the same block
SVX_DFL_HD DynCtx carve_dyn(uint8_t* lds, const Ctx& c, uint8_t* ws)
{
    DynCtx d;
    d.hist_lit = reinterpret_cast<uint32_t*>(lds + LDS_BYTES);
    d.hist_dist = d.hist_lit + NLIT;
    uint8_t* q = reinterpret_cast<uint8_t*>(c.table);
    d.stage2 = reinterpret_cast<uint32_t*>(q); q += 4u * STAGE2_WORDS;
    d.ds = reinterpret_cast<uint32_t*>(q); q += 4u * D_WORDS;
    q = carve_huff(&d.lit, q, NLIT, CODE_BITS);
    q = carve_huff(&d.dist, q, NDIST, CODE_BITS);
    q = carve_huff(&d.cl, q, NCL_ROOM, CL_BITS);
    d.seq_sym = q; q += SEQ_ROOM;
    d.seq_ext = q;
    d.ws_tok = ws;
    d.ws_mark = reinterpret_cast<uint32_t*>(ws + MAX_IN);
    return d;
}

SVX_DFL_HD uint32_t fixed_len(uint32_t sym) { return sym < 144u ? 8u : sym < 256u ? 9u : sym < 280u ? 7u : 8u; }
SVX_DFL_HD uint32_t len_extra(uint32_t sym) { return sym >= 265u && sym < 285u ? (sym - 261u) / 4u : 0u; }
SVX_DFL_HD uint32_t dist_extra(uint32_t sym) { return sym >= 4u ? sym / 2u - 1u : 0u; }
SVX_DFL_HD uint32_t seq_extra(uint32_t sym) { return sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u; }

// h.w [n] -> h.len [n]: a complete length-limited code over the symbols of weight > 0, at least two of them
template <class E>
SVX_DFL_HD void build_code(E& ex, const Huff& h)
{
    const uint32_t N = h.n, maxb = h.maxbits;
    ex.each([&](uint32_t t) {
        if (t < ST_WORDS) h.st[t] = 0;
        if (t < N) h.len[t] = 0;
    });
    ex.barrier();
    ex.each([&](uint32_t t) {
        if (t < N && h.w[t]) { ex.atomic_add(&h.st[ST_USED], 1u); ex.atomic_max(&h.st[ST_TOP], t + 1u); }
    });
    ex.barrier();
    ex.each([&](uint32_t t) {
        if (t == 0) {                                // zlib's stand-ins: the symbol behind the highest used one while that is below 2, else 0
            uint32_t used = h.st[ST_USED], top = h.st[ST_TOP];
            while (used < 2u) { const uint32_t node = top < 3u ? top++ : 0u; h.w[node] = 1; ++used; }
            h.st[ST_USED] = used;
        }
    });
    ex.barrier();
    // ---- rank by (weight, symbol)
    ex.each([&](uint32_t t) {
        if (t < N && h.w[t]) {
            const uint32_t mine = h.w[t];
            uint32_t r = 0;
            for (uint32_t s = 0; s < N; ++s) { const uint32_t o = h.w[s]; if (o && (o < mine || (o == mine && s < t))) ++r; }
            h.order[r] = (uint16_t)t;
            h.sw[r] = mine;
        }
    });
    ex.barrier();
    // ---- Huffman's merge: the leaves by rank and the nodes by birth are two sorted queues
    ex.each([&](uint32_t t) {
        if (t == 0) {
            const uint32_t m = h.st[ST_USED];
            uint32_t li = 0, ni = 0;
            for (uint32_t nn = 0; nn + 1u < m; ++nn) {
                uint32_t f = 0;
                for (int k = 0; k < 2; ++k) {
                    if (li < m && (ni >= nn || h.sw[li] <= h.nfreq[ni])) { f += h.sw[li]; h.parent[li] = (uint16_t)(N + nn); ++li; }
                    else { f += h.nfreq[ni]; h.parent[N + ni] = (uint16_t)(N + nn); ++ni; }
                }
                h.nfreq[nn] = f;
            }
        }
    });
    ex.barrier();
    // ---- depths, counted per length with the limit as the last bin
    ex.each([&](uint32_t t) {
        const uint32_t m = h.st[ST_USED];
        if (t < m) {
            const uint32_t root = N + m - 2u;
            uint32_t x = t, dep = 0;
            while (x != root && dep < N) { x = h.parent[x]; ++dep; }
            ex.atomic_add(&h.st[dep < maxb ? dep : maxb], 1u);
        }
    });
    ex.barrier();
    // ---- the limit's repair: the Kraft sum in units of 2^-maxb is above 2^maxb by one for every step to take
    ex.each([&](uint32_t t) {
        if (t == 0) {
            uint32_t k = 0;
            for (uint32_t l = 1; l <= maxb; ++l) k += h.st[l] << (maxb - l);
            for (uint32_t over = k > (1u << maxb) ? k - (1u << maxb) : 0u; over; --over) {
                uint32_t bits = maxb - 1u;
                while (bits && h.st[bits] == 0) --bits;
                if (!bits || !h.st[maxb]) break;
                h.st[bits] -= 1u; h.st[bits + 1u] += 2u; h.st[maxb] -= 1u;
            }
        }
    });
    ex.barrier();
    // ---- the lengths by rank: the lightest symbols get the longest codes
    ex.each([&](uint32_t t) {
        if (t < h.st[ST_USED]) {
            uint32_t acc = 0, got = 0;
            for (uint32_t l = maxb; l >= 1u && !got; --l) { if (t < acc + h.st[l]) got = l; acc += h.st[l]; }
            h.len[h.order[t]] = (uint8_t)got;
        }
    });
    ex.barrier();
}

// h.len [n] -> h.code [n]: the canonical code (RFC 1951, 3.2.2), bit-reversed for the LSB-first stream
template <class E>
SVX_DFL_HD void assign_codes(E& ex, const Huff& h)
{
    const uint32_t N = h.n;
    ex.each([&](uint32_t t) { if (t < ST_WORDS) h.st[t] = 0; });
    ex.barrier();
    ex.each([&](uint32_t t) { if (t < N && h.len[t]) ex.atomic_add(&h.st[h.len[t]], 1u); });
    ex.barrier();
    ex.each([&](uint32_t t) {
        if (t < N && h.len[t]) {
            const uint32_t L = h.len[t];
            uint32_t code = 0;
            for (uint32_t b = 1; b <= L; ++b) code = (code + (b > 1u ? h.st[b - 1u] : 0u)) << 1;
            for (uint32_t s = 0; s < t; ++s) code += h.len[s] == L;
            h.code[t] = (uint16_t)rev_bits(code, L);
        }
    });
    ex.barrier();
}

// (one lane) the lengths len[0 .. cnt) appended to the code-length sequence the way zlib's send_tree runs them, counted into cl.w
SVX_DFL_HD uint32_t run_lengths(const DynCtx& d, const uint8_t* len, uint32_t cnt, uint32_t at)
{
    uint32_t prev = 0xFFFFu, next = len[0], count = 0, maxc = next ? 7u : 138u, minc = next ? 4u : 3u;
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t cur = next;
        next = i + 1u < cnt ? len[i + 1u] : 0xFFFFu;
        if (++count < maxc && cur == next) continue;
        if (count < minc) {
            for (uint32_t k = 0; k < count; ++k) { d.seq_sym[at] = (uint8_t)cur; d.seq_ext[at] = 0; ++at; }
            d.cl.w[cur] += count;
        } else if (cur != 0) {
            if (cur != prev) { d.seq_sym[at] = (uint8_t)cur; d.seq_ext[at] = 0; ++at; d.cl.w[cur] += 1u; --count; }
            d.seq_sym[at] = 16; d.seq_ext[at] = (uint8_t)(count - 3u); ++at; d.cl.w[16] += 1u;
        } else if (count <= 10u) {
            d.seq_sym[at] = 17; d.seq_ext[at] = (uint8_t)(count - 3u); ++at; d.cl.w[17] += 1u;
        } else {
            d.seq_sym[at] = 18; d.seq_ext[at] = (uint8_t)(count - 11u); ++at; d.cl.w[18] += 1u;
        }
        count = 0; prev = cur;
        if (next == 0) { maxc = 138; minc = 3; } else if (cur == next) { maxc = 6; minc = 3; } else { maxc = 7; minc = 4; }
    }
    return at;
}

// the halves in cand (first) and keys (second), the first half's bits in mlen (0: the thread has nothing), both halves' in tokoff:
// behind s[S_BITS] into the staging area, its whole bytes to the member, the open byte carried
template <class E>
SVX_DFL_HD void put_halves(E& ex, const Ctx& c, const DynCtx& d, uint8_t* slot, uint32_t cap)
{
    uint32_t total = 0;
    ex.scan(c.tokoff, &total);
    ex.each([&](uint32_t t) {
        if (c.mlen[t]) {
            const uint32_t o = (c.s[S_BITS] & 7u) + c.tokoff[t], o2 = o + c.mlen[t];
            const uint64_t v = (uint64_t)c.cand[t] << (o & 31u), v2 = (uint64_t)c.keys[t] << (o2 & 31u);
            if ((uint32_t)v) ex.atomic_or(&d.stage2[o >> 5], (uint32_t)v);
            if ((uint32_t)(v >> 32)) ex.atomic_or(&d.stage2[(o >> 5) + 1u], (uint32_t)(v >> 32));
            if ((uint32_t)v2) ex.atomic_or(&d.stage2[o2 >> 5], (uint32_t)v2);
            if ((uint32_t)(v2 >> 32)) ex.atomic_or(&d.stage2[(o2 >> 5) + 1u], (uint32_t)(v2 >> 32));
        }
    });
    ex.barrier();
    ex.each([&](uint32_t t) {
        const uint32_t bits = c.s[S_BITS], base = bits >> 3, nfull = ((bits & 7u) + total) >> 3;
        for (uint32_t k = t; k < nfull; k += T)
            if (base + k < cap) slot[HEADER + base + k] = (uint8_t)(d.stage2[k >> 2] >> (8u * (k & 3u)));
        if (t == 0) c.s[S_LEFT] = (d.stage2[nfull >> 2] >> (8u * (nfull & 3u))) & 255u;
    });
    ex.barrier();
    ex.each([&](uint32_t t) {
        for (uint32_t i = t; i < STAGE2_WORDS; i += T) d.stage2[i] = i == 0 ? c.s[S_LEFT] : 0u;
    });
    ex.barrier();
    ex.each([&](uint32_t t) { if (t == 0) c.s[S_BITS] += total; });
    ex.barrier();
}

// One block in the smallest of the three forms.  src [n] -> slot [18 + min(n + 5, fixed, dynamic) + 8], *member_len, *btype (0, 1 or
// 2).  d.ws_tok / d.ws_mark: the block's part of the workspace.  The CRC32's 4 bytes at member_len - 8 are left for the caller.
template <class E>
SVX_DFL_HD void encode_block_dyn(E& ex, const Ctx& c, const DynCtx& d, const uint8_t* src, uint32_t n, uint8_t* slot, uint32_t* member_len,
                                 uint32_t* btype)
{
    const uint32_t cap = n + STORED_EXTRA;
    ex.tick(0);
    load_block(ex, c, src, n);
    ex.each([&](uint32_t t) {
        if (t < NLIT) d.hist_lit[t] = t == EOB ? 1u : 0u;            // the end-of-block symbol is every block's
        if (t < NDIST) d.hist_dist[t] = 0;
        if (t == 0) c.s[S_START] = 0;
    });
    ex.barrier();
    for (uint32_t tile = 0; tile < n; tile += T) {
        const uint32_t cnt = n - tile < T ? n - tile : T;
        parse_tile(ex, c, n, tile, cnt);
        // ---- record
        ex.each([&](uint32_t t) {
            if (t < cnt && c.mark[t]) {
                const uint32_t len = c.mlen[t], p = tile + t;
                if (len == 0) ex.atomic_add(&d.hist_lit[c.in[p]], 1u);
                else {
                    uint32_t le, lx, de, dx;
                    ex.atomic_add(&d.hist_lit[len_symbol(len, &le, &lx)], 1u);
                    ex.atomic_add(&d.hist_dist[dist_symbol((uint32_t)c.mdist[t] + 1u, &de, &dx)], 1u);
                    const uint32_t v = (len - 3u) | (uint32_t)c.mdist[t] << 8;
                    d.ws_tok[p] = (uint8_t)v; d.ws_tok[p + 1u] = (uint8_t)(v >> 8); d.ws_tok[p + 2u] = (uint8_t)(v >> 16);
                }
                if (t + (len ? len : 1u) >= cnt) c.s[S_START] = tile + t + (len ? len : 1u);
            }
            if (32u * t < cnt) {                     // (mark is 0 from cnt on)
                uint32_t w = 0;
                for (uint32_t j = 0; j < 32u; ++j) w |= (uint32_t)(c.mark[32u * t + j] & 1u) << j;
                d.ws_mark[(tile >> 5) + t] = w;
            }
        });
        ex.barrier();
    }
    ex.tick(1);
    // ---- codes
    ex.each([&](uint32_t t) {
        if (t < NLIT) d.lit.w[t] = d.hist_lit[t];
        if (t < NDIST) { d.dist.w[t] = d.hist_dist[t]; d.cl.w[t] = 0; }
        if (t < D_WORDS) d.ds[t] = 0;
    });
    ex.barrier();
    build_code(ex, d.lit);
    build_code(ex, d.dist);
    ex.each([&](uint32_t t) {
        if (t == 0) {
            uint32_t hl = USED_LIT, hd = USED_DIST;
            while (hl > 257u && d.lit.len[hl - 1u] == 0) --hl;
            while (hd > 1u && d.dist.len[hd - 1u] == 0) --hd;
            d.ds[D_HLIT] = hl; d.ds[D_HDIST] = hd;
            d.ds[D_SEQ] = run_lengths(d, d.dist.len, hd, run_lengths(d, d.lit.len, hl, 0));
        }
    });
    ex.barrier();
    build_code(ex, d.cl);
    // ---- the choice
    ex.each([&](uint32_t t) {
        if (t < NLIT && d.hist_lit[t]) {
            ex.atomic_add(&d.ds[D_DYN], d.hist_lit[t] * (d.lit.len[t] + len_extra(t)));
            ex.atomic_add(&d.ds[D_FIX], d.hist_lit[t] * (fixed_len(t) + len_extra(t)));
        }
        if (t >= NLIT && t < NLIT + NDIST && d.hist_dist[t - NLIT]) {
            const uint32_t s = t - NLIT;
            ex.atomic_add(&d.ds[D_DYN], d.hist_dist[s] * (d.dist.len[s] + dist_extra(s)));
            ex.atomic_add(&d.ds[D_FIX], d.hist_dist[s] * (5u + dist_extra(s)));
        }
        if (t < d.ds[D_SEQ]) ex.atomic_add(&d.ds[D_DYN], d.cl.len[d.seq_sym[t]] + seq_extra(d.seq_sym[t]));
    });
    ex.barrier();
    ex.each([&](uint32_t t) {
        if (t == 0) {
            const uint8_t ord[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint32_t hc = NCL;
            while (hc > 4u && d.cl.len[ord[hc - 1u]] == 0) --hc;
            d.ds[D_HCLEN] = hc;
            const uint32_t dyn = (3u + 14u + 3u * hc + d.ds[D_DYN] + 7u) >> 3, fixed = (3u + d.ds[D_FIX] + 7u) >> 3;
            const uint32_t form = cap <= fixed && cap <= dyn ? FORM_STORED : fixed <= dyn ? FORM_FIXED : FORM_DYNAMIC;
            d.ds[D_FORM] = form;
            d.ds[D_PAYLOAD] = form == FORM_STORED ? cap : form == FORM_FIXED ? fixed : dyn;
        }
    });
    ex.barrier();
    const uint32_t form = d.ds[D_FORM];
    ex.tick(2);
    if (form != FORM_STORED) {
        // ---- emit: the tables, the header, the tokens
        ex.each([&](uint32_t t) {
            if (form == FORM_FIXED) {
                if (t < NLIT) d.lit.len[t] = (uint8_t)fixed_len(t);
                if (t < NDIST) d.dist.len[t] = 5;
            }
            for (uint32_t i = t; i < STAGE2_WORDS; i += T) d.stage2[i] = 0;
        });
        ex.barrier();
        assign_codes(ex, d.lit);
        assign_codes(ex, d.dist);
        assign_codes(ex, d.cl);
        ex.each([&](uint32_t t) {
            if (t == 0) {
                if (form == FORM_FIXED) { d.stage2[0] = 3; c.s[S_BITS] = 3; }     // BFINAL 1, BTYPE 01
                else {
                    const uint8_t ord[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
                    const uint32_t hc = d.ds[D_HCLEN];
                    uint32_t at = 17, pro[3] = {0, 0, 0};      // BFINAL 1, BTYPE 10, HLIT, HDIST, HCLEN; 17 + 3 x 19 bits at most
                    pro[0] = 5u | (d.ds[D_HLIT] - 257u) << 3 | (d.ds[D_HDIST] - 1u) << 8 | (hc - 4u) << 13;
                    for (uint32_t k = 0; k < hc; ++k, at += 3u) {
                        const uint64_t v = (uint64_t)d.cl.len[ord[k]] << (at & 31u);
                        pro[at >> 5] |= (uint32_t)v;
                        if ((uint32_t)(v >> 32)) pro[(at >> 5) + 1u] |= (uint32_t)(v >> 32);
                    }
                    for (uint32_t k = 0; k < at >> 3; ++k)   // its whole bytes to the member, the open byte to the staging area
                        if (k < cap) slot[HEADER + k] = (uint8_t)(pro[k >> 2] >> (8u * (k & 3u)));
                    d.stage2[0] = (pro[at >> 5] >> (at & 24u)) & 255u;
                    c.s[S_BITS] = at;
                }
            }
        });
        ex.barrier();
        if (form == FORM_DYNAMIC) {
            ex.each([&](uint32_t t) {
                uint32_t lo = 0, hi = 0, nlo = 0, nb = 0;
                if (t < d.ds[D_SEQ]) {
                    const uint32_t sym = d.seq_sym[t];
                    lo = d.cl.code[sym]; nlo = d.cl.len[sym]; hi = d.seq_ext[t]; nb = nlo + seq_extra(sym);
                }
                c.cand[t] = lo; c.keys[t] = hi; c.mlen[t] = (uint16_t)nlo; c.tokoff[t] = nb;
            });
            put_halves(ex, c, d, slot, cap);
        }
        for (uint32_t tile = 0; tile < n; tile += T) {
            ex.each([&](uint32_t t) {
                const uint32_t p = tile + t;
                uint32_t lo = 0, hi = 0, nlo = 0, nb = 0;
                if (p < n && (d.ws_mark[p >> 5] >> (p & 31u) & 1u)) {
                    if (p + 1u >= n || (d.ws_mark[(p + 1u) >> 5] >> ((p + 1u) & 31u) & 1u)) { lo = d.lit.code[c.in[p]]; nlo = nb = d.lit.len[c.in[p]]; }
                    else {
                        const uint32_t v = (uint32_t)d.ws_tok[p] | (uint32_t)d.ws_tok[p + 1u] << 8 | (uint32_t)d.ws_tok[p + 2u] << 16;
                        uint32_t le, lx, de, dx;
                        const uint32_t sym = len_symbol((v & 255u) + 3u, &le, &lx), dsym = dist_symbol((v >> 8) + 1u, &de, &dx);
                        lo = d.lit.code[sym] | lx << d.lit.len[sym]; nlo = d.lit.len[sym] + le;
                        hi = d.dist.code[dsym] | dx << d.dist.len[dsym]; nb = nlo + d.dist.len[dsym] + de;
                    }
                }
                c.cand[t] = lo; c.keys[t] = hi; c.mlen[t] = (uint16_t)nlo; c.tokoff[t] = nb;
            });
            put_halves(ex, c, d, slot, cap);
        }
        // ---- end of block
        ex.each([&](uint32_t t) {
            if (t == 0) {
                const uint32_t bits = c.s[S_BITS], base = bits >> 3, end = (bits + d.lit.len[EOB] + 7u) >> 3;
                const uint32_t v = d.stage2[0] | (uint32_t)d.lit.code[EOB] << (bits & 7u);
                for (uint32_t k = base; k < end; ++k)
                    if (k < cap) slot[HEADER + k] = (uint8_t)(v >> (8u * (k - base)));
                d.ds[D_END] = end;
            }
        });
        ex.barrier();
    }
    close_member(ex, c, n, slot, form == FORM_STORED, d.ds[D_PAYLOAD], member_len);
    ex.each([&](uint32_t t) { if (t == 0) *btype = form; });
    ex.tick(3);
}

}  // namespace svx_dfl
