// svx_sam_core.hpp -- SAM text -> BAM records, the phases of svx_sam.hip, host- and device-compilable: the host program
// tools/hostwave/sam_main.cpp runs this very code, lane by lane and wave by wave, under AddressSanitizer.  The rules are those of
// svision_amd/io/sam.py (its docstring lists them); that module is the yardstick.
//
// lines    count_newlines / emit_newlines: a thread's 16 bytes of a tile of TILE bytes.  The count of every tile, an exclusive
//          prefix over the tiles (the caller's), the emit: line_off[r + 1] = p + 1 for the newline at p of rank r.  No atomics.
// record   ONE WAVE a line.  E is the wave as the phases see it: each(f) runs f(lane) for its 64 lanes, ballot(f) -> the mask of
//          the lanes where f(lane) holds, sum(f) -> the sum of f(lane).  Everything between those calls is the same in every lane
//          (the device: uniform values; the host model: plain locals).  No per-lane value lives across two calls.
//            fields   the first eleven tabs from ballots over 64-byte steps
//            core     FLAG RNAME POS MAPQ RNEXT PNEXT TLEN: a few bytes each, parsed the same in every lane; the reference names
//                     through a table sorted by FNV-1a hash, the bytes compared
//            CIGAR    64 bytes a step: the lanes that hold a letter read their length backwards from it (at most 10 bytes, never
//                     in front of the field), popcount of the letters below = the operation's index.  Measuring needs no index:
//                     there every lane walks its own bytes, 64 apart, and the wave meets in two sums
//            SEQ QUAL 16 text bytes a lane and step
//            tags     the tabs bound the fields (64-byte steps); Z and H copied 64 bytes a step; a B array 64 bytes a step, the lane
//                     that holds a comma parses the value behind it (at most VALUE_MAX bytes, never behind the field), popcount of
//                     the commas below = the value's index
//          record<false> measures: the record's bytes, or a negative code.  record<true> writes what record<false> measured and
//          nothing else: every store lies in out[0 .. len).
// pack     ONE WAVE a line, the same E: pack_measure -> the line's fields and the sizes of its CIGAR words, name and SEQ (or a code);
//          pack_extract_line writes them into the caller's packed arrays, the arrays of svx_bam_walk_extract(_seq) -- no BAM record
//          in between, the tags never read.  The host program tools/hostwave/sam_pack_main.cpp runs these.  At the end of the file.
// Every loop is bounded by the line's [lo, hi); reads reach at most 15 bytes behind hi (the 16-byte loads of SEQ and QUAL).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SVX_SAM_HD __host__ __device__ __forceinline__
#else
#define SVX_SAM_HD inline
#endif

namespace svx_sam {

constexpr uint32_t WAVE = 64;
constexpr uint32_t THREADS = 256, TILE = THREADS * 16;          // the line kernels: a thread's 16 bytes, a workgroup's tile
constexpr uint32_t SLACK = 64;                                  // readable bytes behind the chunk
constexpr uint32_t VALUE_MAX = 40;                              // text bytes of one number the kernels read
constexpr uint32_t MAX_OPS = 65535;
constexpr int32_t HOST = -1, E_FIELDS = -2, E_NUMBER = -3, E_NAME = -4, E_RNAME = -5, E_CIGAR = -6, E_QUAL = -7, E_TAG = -8, E_RANGE = -9,
                  E_HEADER = -10;

struct RefTable {                                               // the @SQ names: hash [n] ascending, tid [n] in that order,
    const uint32_t* hash; const int32_t* tid;                   // name_off [n + 1] and names by tid
    const uint32_t* name_off; const uint8_t* names; uint32_t n;
};
struct Fields { int32_t tid, pos, flag, span; };

// ---- lines ----
SVX_SAM_HD uint32_t newline_mask(const uint8_t* text, uint64_t n, uint64_t at)       // bit j: text[at + j] is a newline, at + j < n
{
    uint8_t b[16];
    memcpy(b, text + at, 16);                                   // (at < n: inside the chunk and its slack)
    uint32_t m = 0;
    for (uint32_t j = 0; j < 16; ++j) m |= (uint32_t)(at + j < n && b[j] == '\n') << j;
    return m;
}
SVX_SAM_HD uint32_t popc32(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
SVX_SAM_HD uint32_t popc64(uint64_t v) { return (uint32_t)__builtin_popcountll(v); }
SVX_SAM_HD uint32_t ctz64(uint64_t v) { return (uint32_t)__builtin_ctzll(v); }

SVX_SAM_HD uint32_t count_newlines(const uint8_t* text, uint64_t n, uint64_t tile, uint32_t t)
{
    const uint64_t at = tile * TILE + (uint64_t)t * 16;
    return at < n ? popc32(newline_mask(text, n, at)) : 0u;
}
// thread t of the tile, `rank` newlines in front of its bytes: a line starts behind every newline.  Entries at or beyond cap are dropped.
SVX_SAM_HD void emit_newlines(const uint8_t* text, uint64_t n, uint64_t tile, uint32_t t, uint64_t rank, int64_t* line_off, uint64_t cap)
{
    const uint64_t at = tile * TILE + (uint64_t)t * 16;
    if (at >= n) return;
    for (uint32_t m = newline_mask(text, n, at); m; m &= m - 1) {
        ++rank;
        if (rank < cap) line_off[rank] = (int64_t)(at + (uint32_t)__builtin_ctz(m) + 1);
    }
}

// ---- numbers (the same in every lane, or a lane's own value of a B array) ----
SVX_SAM_HD bool is_digit(uint8_t c) { return (uint8_t)(c - '0') < 10; }

// [-]digits, 1 to 11 of them
SVX_SAM_HD bool parse_int(const uint8_t* text, uint64_t s, uint64_t e, int64_t* v)
{
    const bool neg = s < e && text[s] == '-';
    s += neg;
    if (e <= s || e - s > 11) return false;
    int64_t a = 0;
    for (uint64_t p = s; p < e; ++p) {
        if (!is_digit(text[p])) return false;
        a = a * 10 + (text[p] - '0');
    }
    *v = neg ? -a : a;
    return true;
}
SVX_SAM_HD int32_t parse_ranged(const uint8_t* text, uint64_t s, uint64_t e, int64_t lo, int64_t hi, int64_t* v, int32_t range_code = E_NUMBER)
{
    if (!parse_int(text, s, e, v)) return E_NUMBER;
    return *v < lo || *v > hi ? range_code : 0;
}

// The exact fast path of a decimal: at most 15 significant digits and a decimal exponent of magnitude <= 22 -- one IEEE multiply or
// divide of two exactly representable doubles, then the cast.  Everything else (longer, inf, nan, not a number): false.
SVX_SAM_HD bool parse_float(const uint8_t* text, uint64_t s, uint64_t e, float* out)
{
    const double P[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20,
                          1e21, 1e22};
    if (e <= s || e - s > VALUE_MAX) return false;
    bool neg = false;
    if (text[s] == '-' || text[s] == '+') { neg = text[s] == '-'; ++s; }
    uint64_t m = 0;
    int32_t digits = 0, sig = 0, frac = 0, ex = 0;
    bool point = false;
    for (; s < e; ++s) {
        const uint8_t c = text[s];
        if (is_digit(c)) {
            ++digits;
            if (m != 0 || c != '0') { if (++sig > 15) return false; }
            m = m * 10 + (uint64_t)(c - '0');
            frac += point;
        } else if (c == '.' && !point) point = true;
        else break;
    }
    if (digits == 0) return false;
    if (s < e) {
        if (text[s] != 'e' && text[s] != 'E') return false;
        ++s;
        bool eneg = false;
        if (s < e && (text[s] == '-' || text[s] == '+')) { eneg = text[s] == '-'; ++s; }
        if (e <= s || e - s > 4) return false;
        for (; s < e; ++s) {
            if (!is_digit(text[s])) return false;
            ex = ex * 10 + (text[s] - '0');
        }
        if (eneg) ex = -ex;
    }
    ex -= frac;
    if (ex < -22 || ex > 22) return false;
    const double d = ex < 0 ? (double)m / P[-ex] : (double)m * P[ex];
    *out = (float)(neg ? -d : d);
    return true;
}

SVX_SAM_HD void put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
SVX_SAM_HD void put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
SVX_SAM_HD void put_float(uint8_t* p, float f) { uint32_t u; memcpy(&u, &f, 4); put32(p, u); }

// -> tid, -1 for `*`, -2 for a name the table does not hold
SVX_SAM_HD int32_t ref_lookup(const uint8_t* text, uint64_t s, uint64_t e, const RefTable& rt)
{
    if (e - s == 1 && text[s] == '*') return -1;
    uint32_t h = 0x811C9DC5u;
    for (uint64_t p = s; p < e; ++p) h = (h ^ text[p]) * 0x01000193u;
    uint32_t lo = 0, hi = rt.n;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (rt.hash[mid] < h) lo = mid + 1; else hi = mid; }
    for (; lo < rt.n && rt.hash[lo] == h; ++lo) {
        const int32_t t = rt.tid[lo];
        const uint32_t a = rt.name_off[t], b = rt.name_off[t + 1];
        if (b - a != e - s) continue;
        bool same = true;
        for (uint32_t k = 0; k < b - a && same; ++k) same = rt.names[a + k] == text[s + k];
        if (same) return t;
    }
    return -2;
}

SVX_SAM_HD int32_t reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (int32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int32_t)(1 + (beg >> 26));
    return 0;
}

// the operation whose letter is at p of the CIGAR that starts at s -> len << 4 | op; ~0: not an operation
SVX_SAM_HD uint32_t cigar_word(const uint8_t* text, uint64_t s, uint64_t p)
{
    uint32_t op;
    switch (text[p]) {
        case 'M': op = 0; break; case 'I': op = 1; break; case 'D': op = 2; break; case 'N': op = 3; break; case 'S': op = 4; break;
        case 'H': op = 5; break; case 'P': op = 6; break; case '=': op = 7; break; case 'X': op = 8; break;
        default: return ~0u;
    }
    uint64_t len = 0, scale = 1;
    uint32_t k = 0;
    for (; k < 10 && p - k > s && is_digit(text[p - k - 1]); ++k, scale *= 10) len += scale * (uint64_t)(text[p - k - 1] - '0');
    if (k < 1 || k > 9 || len >= (1u << 28)) return ~0u;
    return (uint32_t)len << 4 | op;
}

// 4 bits a base by =ACMGRSVTWYHKDBN, either case, N for every other byte: two words of nibbles indexed by the letter's place
SVX_SAM_HD uint32_t base_code(uint8_t c)
{
    if (c == '=') return 0;
    if ((uint8_t)((c | 32) - 'a') >= 26) return 15;
    const uint32_t i = c & 31u;
    return (uint32_t)((i < 16 ? 0xFF3FCFFB4FFD2E1Full >> (4 * i) : 0xFFFFFFAF97F865FFull >> (4 * (i - 16))) & 15u);
}

SVX_SAM_HD uint32_t b_size(uint8_t sub)
{
    switch (sub) { case 'c': case 'C': return 1; case 's': case 'S': return 2; case 'i': case 'I': case 'f': return 4; default: return 0; }
}

// the first tab of text[from .. hi), or hi
template <class E>
SVX_SAM_HD uint64_t next_tab(E& ex, const uint8_t* text, uint64_t from, uint64_t hi)
{
    for (uint64_t at = from; at < hi; at += WAVE) {
        const uint64_t m = ex.ballot([&](uint32_t l) { return at + l < hi && text[at + l] == '\t'; });
        if (m) return at + ctz64(m);
    }
    return hi;
}

// bytes text[s .. e) -> to, 64 a step
template <class E>
SVX_SAM_HD void copy_text(E& ex, const uint8_t* text, uint64_t s, uint64_t e, uint8_t* to)
{
    for (uint64_t at = s; at < e; at += WAVE)
        ex.each([&](uint32_t l) { if (at + l < e) to[at + l - s] = text[at + l]; });
}

// One tag field text[ts .. te) -> its BAM bytes (a negative code), written to `to` where WRITE.
template <bool WRITE, class E>
SVX_SAM_HD int64_t tag(E& ex, const uint8_t* text, uint64_t ts, uint64_t te, uint8_t* to)
{
    if (te - ts < 5 || text[ts + 2] != ':' || text[ts + 4] != ':') return E_TAG;
    const uint8_t typ = text[ts + 3];
    const uint64_t vs = ts + 5;
    uint8_t out_typ = typ;
    int64_t size;
    if (typ == 'A') {
        if (te - vs != 1) return E_TAG;
        size = 4;
        if (WRITE) ex.each([&](uint32_t l) { if (l == 0) to[3] = text[vs]; });
    } else if (typ == 'Z' || typ == 'H') {
        size = 3 + (int64_t)(te - vs) + 1;
        if (WRITE) {
            copy_text(ex, text, vs, te, to + 3);
            ex.each([&](uint32_t l) { if (l == 0) to[size - 1] = 0; });
        }
    } else if (typ == 'i') {
        int64_t v;
        const int32_t rc = parse_ranged(text, vs, te, -(1ll << 31), (1ll << 32) - 1, &v, E_RANGE);
        if (rc) return rc;
        const uint32_t w = v < 0 ? (v >= -128 ? 1 : v >= -32768 ? 2 : 4) : (v <= 255 ? 1 : v <= 65535 ? 2 : 4);
        out_typ = (uint8_t)(v < 0 ? (w == 1 ? 'c' : w == 2 ? 's' : 'i') : (w == 1 ? 'C' : w == 2 ? 'S' : 'I'));
        size = 3 + w;
        if (WRITE) ex.each([&](uint32_t l) { if (l < w) to[3 + l] = (uint8_t)((uint64_t)v >> (8 * l)); });
    } else if (typ == 'f') {
        float f;
        if (!parse_float(text, vs, te, &f)) return HOST;
        size = 7;
        if (WRITE) ex.each([&](uint32_t l) { if (l == 0) put_float(to + 3, f); });
    } else if (typ == 'B') {
        if (te == vs || (te - vs > 1 && text[vs + 1] != ',')) return E_TAG;
        const uint8_t sub = text[vs];
        const uint32_t esize = b_size(sub);
        if (!esize) return E_TAG;
        int64_t lo = 0, hi = 0;
        switch (sub) {
            case 'c': lo = -128; hi = 127; break; case 'C': hi = 255; break; case 's': lo = -32768; hi = 32767; break;
            case 'S': hi = 65535; break; case 'i': lo = -(1ll << 31); hi = (1ll << 31) - 1; break; case 'I': hi = (1ll << 32) - 1; break;
        }
        uint64_t count = 0;
        for (uint64_t at = vs + 1; at < te; at += WAVE) {
            const uint64_t commas = ex.ballot([&](uint32_t l) { return at + l < te && text[at + l] == ','; });
            // the lane of a comma takes the value behind it: -> 0, 1 (not the kernels': HOST), 1 << 16 (not a number)
            const uint64_t trouble = ex.sum([&](uint32_t l) -> uint64_t {
                if (!(commas >> l & 1)) return 0;
                const uint64_t s = at + l + 1;
                uint64_t e = s;
                while (e < te && e - s <= VALUE_MAX && text[e] != ',') ++e;
                if (sub == 'f') {
                    float f;
                    if (!parse_float(text, s, e, &f)) return 1;
                    if (WRITE) put_float(to + 8 + (count + popc64(commas & ((1ull << l) - 1))) * 4, f);
                    return 0;
                }
                int64_t v;
                if (parse_ranged(text, s, e, lo, hi, &v)) return 1u << 16;
                if (WRITE) {
                    uint8_t* q = to + 8 + (count + popc64(commas & ((1ull << l) - 1))) * esize;
                    for (uint32_t k = 0; k < esize; ++k) q[k] = (uint8_t)((uint64_t)v >> (8 * k));
                }
                return 0;
            });
            if (trouble >> 16) return E_NUMBER;
            if (trouble) return HOST;
            count += popc64(commas);
        }
        size = 8 + (int64_t)count * esize;
        if (WRITE) ex.each([&](uint32_t l) { if (l == 0) { to[3] = sub; put32(to + 4, (uint32_t)count); } });
    } else return E_TAG;
    if (WRITE) ex.each([&](uint32_t l) { if (l == 0) { to[0] = text[ts]; to[1] = text[ts + 1]; to[2] = out_typ; } });
    return size;
}

// The line text[lo .. hi) (no newline) -> its record's bytes including block_size, or a negative code; *fl where >= 0 or HOST is not
// promised.  WRITE: the record to out[0 .. the same bytes) -- the caller has measured the line and the answer was not negative.
template <bool WRITE, class E>
SVX_SAM_HD int64_t record(E& ex, const uint8_t* text, uint64_t lo, uint64_t hi, const RefTable& rt, uint8_t* out, Fields* fl)
{
    if (lo >= hi) return E_FIELDS;
    if (text[lo] == '@') return E_HEADER;
    // ---- fields: s[k] .. e[k] of the eleven, the tags behind them
    uint64_t s[11], e[11];
    uint32_t n_tab = 0;
    s[0] = lo;
    for (uint64_t at = lo; at < hi && n_tab < 11; at += WAVE) {
        uint64_t m = ex.ballot([&](uint32_t l) { return at + l < hi && text[at + l] == '\t'; });
        for (; m && n_tab < 11; m &= m - 1) {
            const uint64_t p = at + ctz64(m);
            e[n_tab] = p;
            if (++n_tab < 11) s[n_tab] = p + 1;
        }
    }
    if (n_tab < 10) return E_FIELDS;
    if (n_tab == 10) e[10] = hi;
    const bool has_tags = n_tab == 11;
    // ---- core
    const uint64_t l_name = e[0] - s[0];
    if (l_name < 1 || l_name > 254) return E_NAME;
    int64_t flag, pos, mapq, pnext, tlen;
    int32_t rc;
    if ((rc = parse_ranged(text, s[1], e[1], 0, 65535, &flag))) return rc;
    const int32_t tid = ref_lookup(text, s[2], e[2], rt);
    if (tid < -1) return E_RNAME;
    if ((rc = parse_ranged(text, s[3], e[3], 0, 0x7FFFFFFF, &pos))) return rc;
    if ((rc = parse_ranged(text, s[4], e[4], 0, 255, &mapq))) return rc;
    // ---- CIGAR
    const bool no_cigar = e[5] - s[5] == 1 && text[s[5]] == '*';
    uint64_t n_ops = 0, span = 0;
    const uint64_t cigar_at = 36 + l_name + 1;                 // (offsets, not pointers: a measuring call has no `out`)
    if (!no_cigar) {
        if (e[5] == s[5] || is_digit(text[e[5] - 1])) return E_CIGAR;
        if (!WRITE) {
            // measuring wants no operation's index: every lane walks its own bytes of the field, 64 apart, and the wave meets twice
            const uint64_t got = ex.sum([&](uint32_t l) -> uint64_t {
                uint64_t ref = 0;
                for (uint64_t p = s[5] + l; p < e[5]; p += WAVE) {
                    if (is_digit(text[p])) continue;
                    const uint32_t w = cigar_word(text, s[5], p);
                    if (w == ~0u) return 1ull << 56;             // (the lengths of a line's operations add up to less than 2^56)
                    const uint32_t op = w & 15u;
                    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref += w >> 4;
                }
                return ref;
            });
            if (got >> 56) return E_CIGAR;
            span = got;
            n_ops = ex.sum([&](uint32_t l) -> uint64_t {
                uint64_t n = 0;
                for (uint64_t p = s[5] + l; p < e[5]; p += WAVE) n += !is_digit(text[p]);
                return n;
            });
        }
        for (uint64_t at = s[5]; WRITE && at < e[5]; at += WAVE) {
            const uint64_t letters = ex.ballot([&](uint32_t l) { return at + l < e[5] && !is_digit(text[at + l]); });
            // a letter's lane: its reference bases, or 1 << 40 where it is no operation
            const uint64_t got = ex.sum([&](uint32_t l) -> uint64_t {
                if (!(letters >> l & 1)) return 0;
                const uint32_t w = cigar_word(text, s[5], at + l);
                if (w == ~0u) return 1ull << 40;
                if (WRITE) put32(out + cigar_at + 4 * (n_ops + popc64(letters & ((1ull << l) - 1))), w);
                const uint32_t op = w & 15u;
                return op == 0 || op == 2 || op == 3 || op == 7 || op == 8 ? w >> 4 : 0u;
            });
            if (got >> 40) return E_CIGAR;
            span += got;
            n_ops += popc64(letters);
        }
        if (n_ops > MAX_OPS) return HOST;
    }
    int32_t next_tid = tid;
    if (!(e[6] - s[6] == 1 && text[s[6]] == '=')) {
        next_tid = ref_lookup(text, s[6], e[6], rt);
        if (next_tid < -1) return E_RNAME;
    }
    if ((rc = parse_ranged(text, s[7], e[7], 0, 0x7FFFFFFF, &pnext))) return rc;
    if ((rc = parse_ranged(text, s[8], e[8], -0x7FFFFFFFll, 0x7FFFFFFF, &tlen))) return rc;
    // ---- SEQ and QUAL
    const uint64_t l_seq = e[9] - s[9] == 1 && text[s[9]] == '*' ? 0 : e[9] - s[9];
    const bool no_qual = e[10] - s[10] == 1 && text[s[10]] == '*';
    if (!no_qual && e[10] - s[10] != l_seq) return E_QUAL;
    if (l_seq > 0x7FFFFFFF) return E_FIELDS;
    const uint64_t seq_at = cigar_at + 4 * n_ops, qual_at = seq_at + (l_seq + 1) / 2, tags_at = qual_at + l_seq;
    pos -= 1;
    if (fl) { fl->tid = tid; fl->pos = (int32_t)pos; fl->flag = (int32_t)flag; fl->span = (int32_t)(span > 0x7FFFFFFF ? 0x7FFFFFFF : span); }
    if (WRITE) {
        const uint32_t bin = tid < 0 ? 4680u : (uint32_t)reg2bin(pos, pos + (int64_t)(span ? span : 1)) & 0xFFFFu;
        ex.each([&](uint32_t l) {
            if (l == 0) {
                put32(out + 4, (uint32_t)tid); put32(out + 8, (uint32_t)pos);
                out[12] = (uint8_t)(l_name + 1); out[13] = (uint8_t)mapq; put16(out + 14, bin);
                put16(out + 16, (uint32_t)n_ops); put16(out + 18, (uint32_t)flag); put32(out + 20, (uint32_t)l_seq);
                put32(out + 24, (uint32_t)next_tid); put32(out + 28, (uint32_t)(pnext - 1)); put32(out + 32, (uint32_t)tlen);
                out[36 + l_name] = 0;
            }
        });
        copy_text(ex, text, s[0], e[0], out + 36);
        uint8_t* const seq_to = out + seq_at;
        uint8_t* const qual_to = out + qual_at;
        for (uint64_t at = 0; at < l_seq; at += WAVE * 16) {
            ex.each([&](uint32_t l) {
                const uint64_t p = at + (uint64_t)l * 16;
                if (p >= l_seq) return;
                uint8_t b[16];
                memcpy(b, text + s[9] + p, 16);                 // (up to 15 bytes behind the field: the line's own bytes or the slack)
                for (uint32_t j = 0; j < 16 && p + j < l_seq; j += 2)
                    seq_to[(p + j) / 2] = (uint8_t)(base_code(b[j]) << 4 | (p + j + 1 < l_seq ? base_code(b[j + 1]) : 0u));
                if (no_qual) {
                    for (uint32_t j = 0; j < 16 && p + j < l_seq; ++j) qual_to[p + j] = 0xFF;
                } else {
                    memcpy(b, text + s[10] + p, 16);
                    for (uint32_t j = 0; j < 16 && p + j < l_seq; ++j) qual_to[p + j] = (uint8_t)(b[j] - 33);
                }
            });
        }
    }
    // ---- tags
    int64_t l_tags = 0;
    if (has_tags) {
        for (uint64_t ts = e[10] + 1;;) {
            const uint64_t te = next_tab(ex, text, ts, hi);
            const int64_t sz = tag<WRITE>(ex, text, ts, te, WRITE ? out + tags_at + l_tags : nullptr);
            if (sz < 0) return sz;
            l_tags += sz;
            if (te >= hi) break;
            ts = te + 1;
        }
    }
    const int64_t len = 36 + (int64_t)l_name + 1 + 4 * (int64_t)n_ops + (int64_t)((l_seq + 1) / 2) + (int64_t)l_seq + l_tags;
    if (len > 0x7FFFFFFF) return E_FIELDS;
    if (WRITE) ex.each([&](uint32_t l) { if (l == 0) put32(out, (uint32_t)(len - 4)); });
    return len;
}

// the line i of the table: [lo, hi) without its newline
SVX_SAM_HD void line_bounds(const uint8_t* text, const int64_t* line_off, uint64_t i, uint64_t* lo, uint64_t* hi)
{
    *lo = (uint64_t)line_off[i];
    *hi = (uint64_t)line_off[i + 1];
    if (*hi > *lo && text[*hi - 1] == '\n') --*hi;
}

// A wave's line of svx_sam_measure.
template <class E>
SVX_SAM_HD void measure_line(E& ex, const uint8_t* text, const int64_t* line_off, uint64_t i, const RefTable& rt, int32_t* len, int32_t* tid,
                             int32_t* pos, int32_t* flag, int32_t* span)
{
    uint64_t lo, hi;
    line_bounds(text, line_off, i, &lo, &hi);
    Fields f = {-1, -1, 0, 0};
    const int64_t got = record<false>(ex, text, lo, hi, rt, nullptr, &f);
    ex.each([&](uint32_t l) { if (l == 0) { len[i] = (int32_t)got; tid[i] = f.tid; pos[i] = f.pos; flag[i] = f.flag; span[i] = f.span; } });
}

// A wave's line of svx_sam_encode: measured again, and written only where that gives len[i] -- else *status = 1, a plain store.
template <class E>
SVX_SAM_HD void encode_line(E& ex, const uint8_t* text, const int64_t* line_off, uint64_t i, const RefTable& rt, const int32_t* len,
                            const int64_t* off, int64_t out_base, uint8_t* out, int32_t* status)
{
    if (len[i] < 0) return;
    uint64_t lo, hi;
    line_bounds(text, line_off, i, &lo, &hi);
    if (record<false>(ex, text, lo, hi, rt, nullptr, nullptr) != len[i]) {
        ex.each([&](uint32_t l) { if (l == 0) *status = 1; });
        return;
    }
    record<true>(ex, text, lo, hi, rt, out + (off[i] - out_base), nullptr);
}

// ---- pack: a line -> the caller's packed arrays (svx_sam_pack_count / svx_sam_pack_extract), no BAM record in between ----
// What the device ingest keeps of a record (svx_bam_walk_extract(_seq) of the same record): tid pos flag mapq l_seq, the CIGAR words,
// the name and one '\n', the 4-bit SEQ.  The first eleven fields are held to record<>'s rules, in record<>'s order, so a fault there
// has record<>'s code; QUAL is measured, not read; the tags are not looked at; the number of operations has no limit.  The one line
// left to the host (HOST): a CIGAR of the shape <l_seq>S<n>N, the placeholder beside a CG:B:I tag, whose real words are in that tag.
struct Packed { int32_t tid, pos, flag, mapq, l_seq, words, name_bytes, seq_bytes; };

// the bounds s[k] .. e[k] of the first eleven fields -> the tabs seen, at most 11 (10: no tag behind QUAL, e[10] = hi)
template <class E>
SVX_SAM_HD uint32_t split_fields(E& ex, const uint8_t* text, uint64_t lo, uint64_t hi, uint64_t* s, uint64_t* e)
{
    uint32_t n_tab = 0;
    s[0] = lo;
    for (uint64_t at = lo; at < hi && n_tab < 11; at += WAVE) {
        uint64_t m = ex.ballot([&](uint32_t l) { return at + l < hi && text[at + l] == '\t'; });
        for (; m && n_tab < 11; m &= m - 1) {
            const uint64_t p = at + ctz64(m);
            e[n_tab] = p;
            if (++n_tab < 11) s[n_tab] = p + 1;
        }
    }
    if (n_tab == 10) e[10] = hi;
    return n_tab;
}

// The line text[lo .. hi) measured: 0 and *pk, HOST (*pk as the placeholder reads, not for use), or a negative code.
template <class E>
SVX_SAM_HD int32_t pack_measure(E& ex, const uint8_t* text, uint64_t lo, uint64_t hi, const RefTable& rt, bool with_seq, Packed* pk)
{
    if (lo >= hi) return E_FIELDS;
    if (text[lo] == '@') return E_HEADER;
    uint64_t s[11], e[11];
    if (split_fields(ex, text, lo, hi, s, e) < 10) return E_FIELDS;
    const uint64_t l_name = e[0] - s[0];
    if (l_name < 1 || l_name > 254) return E_NAME;
    int64_t flag, pos, mapq, pnext, tlen;
    int32_t rc;
    if ((rc = parse_ranged(text, s[1], e[1], 0, 65535, &flag))) return rc;
    const int32_t tid = ref_lookup(text, s[2], e[2], rt);
    if (tid < -1) return E_RNAME;
    if ((rc = parse_ranged(text, s[3], e[3], 0, 0x7FFFFFFF, &pos))) return rc;
    if ((rc = parse_ranged(text, s[4], e[4], 0, 255, &mapq))) return rc;
    const bool no_cigar = e[5] - s[5] == 1 && text[s[5]] == '*';
    uint64_t n_ops = 0;
    if (!no_cigar) {
        if (e[5] == s[5] || is_digit(text[e[5] - 1])) return E_CIGAR;
        // every lane walks its own bytes of the field, 64 apart: the letters that are no operation, and the letters
        const uint64_t got = ex.sum([&](uint32_t l) -> uint64_t {
            uint64_t n = 0;
            for (uint64_t p = s[5] + l; p < e[5]; p += WAVE) {
                if (is_digit(text[p])) continue;
                if (cigar_word(text, s[5], p) == ~0u) return 1ull << 56;
                ++n;
            }
            return n;
        });
        if (got >> 56) return E_CIGAR;
        n_ops = got;
    }
    if (!(e[6] - s[6] == 1 && text[s[6]] == '=') && ref_lookup(text, s[6], e[6], rt) < -1) return E_RNAME;
    if ((rc = parse_ranged(text, s[7], e[7], 0, 0x7FFFFFFF, &pnext))) return rc;
    if ((rc = parse_ranged(text, s[8], e[8], -0x7FFFFFFFll, 0x7FFFFFFF, &tlen))) return rc;
    const uint64_t l_seq = e[9] - s[9] == 1 && text[s[9]] == '*' ? 0 : e[9] - s[9];
    const bool no_qual = e[10] - s[10] == 1 && text[s[10]] == '*';
    if (!no_qual && e[10] - s[10] != l_seq) return E_QUAL;
    if (l_seq > 0x7FFFFFFF || n_ops > 0x7FFFFFFF) return E_FIELDS;
    pk->tid = tid; pk->pos = (int32_t)(pos - 1); pk->flag = (int32_t)flag; pk->mapq = (int32_t)mapq; pk->l_seq = (int32_t)l_seq;
    pk->words = (int32_t)n_ops; pk->name_bytes = (int32_t)(l_name + 1); pk->seq_bytes = with_seq ? (int32_t)((l_seq + 1) / 2) : 0;
    if (n_ops != 2) return 0;
    // two operations are at most 20 bytes, within one step: the first letter from a ballot.  <l_seq>S<n>N is the host's.
    // KEEP THIS ORDER -- *pk assigned above, the placeholder decided last, by one expression.  An earlier form found the first letter
    // with `while (is_digit(text[p])) ++p;` in FRONT of the assignments and returned HOST from inside that block.  hipcc (ROCm 7.2,
    // -O3, gfx950) compiled it wrongly: in the kernel's ISA the register that held l_seq for the final stores was reused as the zero of
    // the HOST path's merge and not written again on the way back, so a two-operation line that is no placeholder came out with
    // status 0 and l_seq 0.  The source had no undefined behaviour that was found, and the host model ran it right under ASan and
    // UBSan: a compiler fault, as far as it could be read.  The two `two_ops_*` shapes of tests/sam_pack_cases.py hold it down on
    // the device (tests/test_gpu_sam_pack.py); a change here wants that test run, and a look at the stores at the kernel's end.
    const uint64_t letters = ex.ballot([&](uint32_t l) { return s[5] + l < e[5] && !is_digit(text[s[5] + l]); });
    const uint32_t w0 = cigar_word(text, s[5], s[5] + ctz64(letters | 1ull << 63)), w1 = cigar_word(text, s[5], e[5] - 1);
    return (w0 & 15u) == 4 && (w0 >> 4) == l_seq && (w1 & 15u) == 3 ? HOST : 0;
}

// A wave's line of svx_sam_pack_count: status [i]; fields: five planes of n_lines (tid pos flag mapq l_seq), counts: three (CIGAR
// words, name bytes, SEQ bytes) -- zero where the status is not 0.
template <class E>
SVX_SAM_HD void pack_count_line(E& ex, const uint8_t* text, const int64_t* line_off, uint64_t i, uint64_t n_lines, const RefTable& rt,
                                bool with_seq, int32_t* status, int32_t* fields, int32_t* counts)
{
    uint64_t lo, hi;
    line_bounds(text, line_off, i, &lo, &hi);
    Packed pk = {0, 0, 0, 0, 0, 0, 0, 0};
    const int32_t st = pack_measure(ex, text, lo, hi, rt, with_seq, &pk);
    if (st != 0) pk = Packed{0, 0, 0, 0, 0, 0, 0, 0};             // (the host's line: measured, but its counts are the host's to give)
    ex.each([&](uint32_t l) {
        if (l != 0) return;
        status[i] = st;
        fields[i] = pk.tid; fields[n_lines + i] = pk.pos; fields[2 * n_lines + i] = pk.flag; fields[3 * n_lines + i] = pk.mapq;
        fields[4 * n_lines + i] = pk.l_seq;
        counts[i] = pk.words; counts[n_lines + i] = pk.name_bytes; counts[2 * n_lines + i] = pk.seq_bytes;
    });
}

// What svx_sam_pack_extract writes to: element i of the field arrays, and the record's own slots [off[i], off[i + 1]) of the rest.
struct PackOut {
    int32_t* tid; int32_t* pos; int32_t* l_seq; int16_t* flag; uint8_t* mapq;
    const int64_t* cig_off; uint32_t* cigar; const int64_t* name_off; uint8_t* names; const int64_t* seq_off; uint8_t* seq;
};

// A wave's line of svx_sam_pack_extract: a line of status 0 written -- the fields, and the words, name bytes and (o.seq given) SEQ bytes
// into slots of exactly the sizes svx_sam_pack_count gave.  Every store is checked against its slot, so offsets that are not the
// counts' prefix lose data and write nowhere else.  Lines of another status are the caller's.
template <class E>
SVX_SAM_HD void pack_extract_line(E& ex, const uint8_t* text, const int64_t* line_off, uint64_t i, const RefTable& rt, const int32_t* status,
                                  const PackOut& o)
{
    if (status[i] != 0) return;
    uint64_t lo, hi, s[11], e[11];
    line_bounds(text, line_off, i, &lo, &hi);
    if (lo >= hi || split_fields(ex, text, lo, hi, s, e) < 10) return;          // (not a line of status 0)
    int64_t flag = 0, pos = 0, mapq = 0;
    if (parse_ranged(text, s[1], e[1], 0, 65535, &flag) || parse_ranged(text, s[3], e[3], 0, 0x7FFFFFFF, &pos)
        || parse_ranged(text, s[4], e[4], 0, 255, &mapq)) return;
    const int32_t tid = ref_lookup(text, s[2], e[2], rt);
    const uint64_t l_seq = e[9] - s[9] == 1 && text[s[9]] == '*' ? 0 : e[9] - s[9];
    ex.each([&](uint32_t l) {
        if (l != 0) return;
        o.tid[i] = tid; o.pos[i] = (int32_t)(pos - 1); o.l_seq[i] = (int32_t)l_seq; o.flag[i] = (int16_t)(uint16_t)flag; o.mapq[i] = (uint8_t)mapq;
    });
    // ---- the name and its '\n'
    const uint64_t l_name = e[0] - s[0];
    const uint64_t name_room = (uint64_t)(o.name_off[i + 1] - o.name_off[i]);
    if (name_room == l_name + 1) {
        uint8_t* const to = o.names + o.name_off[i];
        copy_text(ex, text, s[0], e[0], to);
        ex.each([&](uint32_t l) { if (l == 0) to[l_name] = '\n'; });
    }
    // ---- the CIGAR words: the lane of a letter, its index the letters in front of it
    if (!(e[5] - s[5] == 1 && text[s[5]] == '*')) {
        const uint64_t room = (uint64_t)(o.cig_off[i + 1] - o.cig_off[i]);
        uint32_t* const to = o.cigar + o.cig_off[i];
        uint64_t n_ops = 0;
        for (uint64_t at = s[5]; at < e[5]; at += WAVE) {
            const uint64_t letters = ex.ballot([&](uint32_t l) { return at + l < e[5] && !is_digit(text[at + l]); });
            ex.each([&](uint32_t l) {
                if (!(letters >> l & 1)) return;
                const uint64_t k = n_ops + popc64(letters & ((1ull << l) - 1));
                if (k < room) to[k] = cigar_word(text, s[5], at + l);
            });
            n_ops += popc64(letters);
        }
    }
    // ---- SEQ: 16 text bytes a lane and step -> 8 bytes, single byte stores (the neighbours' bytes are other waves')
    if (o.seq && l_seq) {
        const uint64_t room = (uint64_t)(o.seq_off[i + 1] - o.seq_off[i]);
        uint8_t* const to = o.seq + o.seq_off[i];
        if (room == (l_seq + 1) / 2) {
            for (uint64_t at = 0; at < l_seq; at += WAVE * 16) {
                ex.each([&](uint32_t l) {
                    const uint64_t p = at + (uint64_t)l * 16;
                    if (p >= l_seq) return;
                    uint8_t b[16];
                    memcpy(b, text + s[9] + p, 16);             // (up to 15 bytes behind the field: the line's own bytes or the slack)
                    for (uint32_t j = 0; j < 16 && p + j < l_seq; j += 2)
                        to[(p + j) / 2] = (uint8_t)(base_code(b[j]) << 4 | (p + j + 1 < l_seq ? base_code(b[j + 1]) : 0u));
                });
            }
        }
    }
}

}  // namespace svx_sam
