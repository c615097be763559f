// lz_table_main.cpp -- bgzf_lz_table_kernel (svision_amd/csrc/svx_lz_table.hip) without a GPU: the phases of
// svx_lz_table_core.hpp -- the code the kernel runs -- as loops over T "threads", against zlib.
//
//   1. A sequential DEFLATE parser writes a block's SPLIT sequence stream the way bgzf_tokens_kernel<true> lays it out: u32
//      headers [literals:8 | match length:9 | distance - 1:15] upwards, the literal bytes downwards from the slot's end; a run of
//      literals is cut at 255, at the end of a DEFLATE block and wherever the kernel's lane segments (512 compressed bits) end.
//   2. build / resolve / emit.  A step of the resolve phase is T threads on T consecutive words; in LOCKSTEP order all reads of
//      a step come before its writes (a wave's view), in FORWARD and REVERSE order every thread writes at once and the threads
//      of a step run first to last / last to first: the kernel's waves are anywhere in between, and all orders must give zlib's
//      bytes (an entry read while its owner updates it is an ancestor either way).
//   3. The output is compared with zlib's.
// Built with -fsanitize=address,undefined: the table, the headers, the literals and the output live in heap blocks of exactly
// their size (the output behind a canary of `ph` bytes -- its neighbour's bytes, which must not change).
//
// usage: lz_table_host [file of BGZF blocks]...    (the crafted sequence streams always run)
//        lz_table_host --count [file]...           the turns of the build's write loops, per block and per file, with every part
//                                                  written by its sequence's thread and with the parts of 16 / 32 / 64 entries or
//                                                  more written by the wave (count_block)
#include <zlib.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../svision_amd/csrc/svx_lz_table_core.hpp"

using namespace svx_lzt;

static const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const uint8_t CLEN_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
enum { HANDOVER = 10 };                                  // svx_inflate2.hip: INF_TOKENS_OVERFLOW, the status of a block left to another kernel
enum Order { LOCKSTEP = 0, FORWARD = 1, REVERSE = 2 };

// ---- 1. DEFLATE -> SPLIT sequence stream (sequential; canonical codes decoded bit by bit)
struct Bits {
    const uint8_t* d; size_t nbits, p = 0; bool bad = false;
    uint32_t get(int n) { uint32_t v = 0; for (int i = 0; i < n; ++i) { if (p >= nbits) { bad = true; return 0; } v |= (uint32_t)((d[p >> 3] >> (p & 7)) & 1) << i; ++p; } return v; }
};
struct Huff {
    uint16_t count[16], symbol[288];
    bool build(const uint8_t* lens, int n)
    {
        memset(count, 0, sizeof count);
        for (int s = 0; s < n; ++s) count[lens[s]]++;
        int left = 1;
        for (int l = 1; l < 16; ++l) { left = (left << 1) - count[l]; if (left < 0) return false; }
        uint16_t offs[16]; offs[1] = 0;
        for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
        for (int s = 0; s < n; ++s) if (lens[s]) symbol[offs[lens[s]]++] = (uint16_t)s;
        return true;
    }
    int decode(Bits& in) const
    {
        int code = 0, first = 0, index = 0;
        for (int l = 1; l < 16; ++l) {
            code |= (int)in.get(1);
            if (in.bad) return -1;
            const int c = count[l];
            if (code - c < first) return symbol[index + (code - first)];
            index += c; first += c; first <<= 1; code <<= 1;
        }
        return -1;
    }
};

struct Split { std::vector<uint32_t> hdr; std::vector<uint8_t> lit; };      // lit[j] = literal j (the slot holds them back to front)

static bool deflate_to_split(const uint8_t* src, size_t n, Split& out)
{
    Bits in{src, n * 8};
    uint32_t nl = 0;
    auto flush = [&] { if (nl) { out.hdr.push_back(nl); nl = 0; } };
    auto literal = [&](uint8_t v) { if (nl == 255) flush(); out.lit.push_back(v); ++nl; };
    bool last = false;
    while (!last) {
        last = in.get(1) != 0;
        const uint32_t type = in.get(2);
        if (in.bad || type == 3) return false;
        if (type == 0) {
            in.p = (in.p + 7) & ~(size_t)7;
            const uint32_t len = in.get(16), nlen = in.get(16);
            if (in.bad || (len ^ nlen) != 0xffffu || in.p + 8ull * len > in.nbits) return false;
            for (uint32_t i = 0; i < len; ++i) literal(src[(in.p >> 3) + i]);
            in.p += 8ull * len;
            flush();
            continue;
        }
        uint8_t lens[320] = {0};
        int nlen_codes = 288, ndist = 30;
        if (type == 1) {
            for (int s = 0; s < 288; ++s) lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
            for (int s = 0; s < 30; ++s) lens[288 + s] = 5;
        } else {
            nlen_codes = (int)in.get(5) + 257; ndist = (int)in.get(5) + 1;
            const int ncode = (int)in.get(4) + 4;
            if (in.bad || nlen_codes > 286 || ndist > 30) return false;
            uint8_t cl[19] = {0};
            for (int i = 0; i < ncode; ++i) cl[CLEN_ORDER[i]] = (uint8_t)in.get(3);
            Huff hc;
            if (in.bad || !hc.build(cl, 19)) return false;
            uint8_t all[320] = {0};
            int i = 0;
            while (i < nlen_codes + ndist) {
                const int sym = hc.decode(in);
                if (sym < 0) return false;
                int value = sym, rep = 1;
                if (sym == 16) { if (i == 0) return false; value = all[i - 1]; rep = 3 + (int)in.get(2); }
                else if (sym == 17) { value = 0; rep = 3 + (int)in.get(3); }
                else if (sym == 18) { value = 0; rep = 11 + (int)in.get(7); }
                if (in.bad || i + rep > nlen_codes + ndist) return false;
                while (rep--) all[i++] = (uint8_t)value;
            }
            if (all[256] == 0) return false;
            memcpy(lens, all, (size_t)nlen_codes);
            memcpy(lens + 288, all + nlen_codes, (size_t)ndist);
        }
        Huff hl, hd;
        if (!hl.build(lens, nlen_codes) || !hd.build(lens + 288, ndist)) return false;
        const size_t start = in.p;
        size_t seg = 0;
        for (;;) {
            if ((in.p - start) / 512 != seg) { seg = (in.p - start) / 512; flush(); }        // a lane segment of the tokens kernel ends
            const int sym = hl.decode(in);
            if (sym < 0) return false;
            if (sym < 256) { literal((uint8_t)sym); continue; }
            if (sym == 256) break;
            if (sym - 257 >= 29) return false;
            const uint32_t len = LEN_BASE[sym - 257] + in.get(LEN_EXTRA[sym - 257]);
            const int ds = hd.decode(in);
            if (ds < 0 || ds >= 30) return false;
            const uint32_t dist = DIST_BASE[ds] + in.get(DIST_EXTRA[ds]);
            if (in.bad) return false;
            out.hdr.push_back(nl | len << 8 | (dist - 1u) << 17);
            nl = 0;
        }
        flush();
    }
    return true;
}

// ---- 2. the kernel's phases on T threads
struct Run { int status = 0; uint32_t rounds = 0; uint64_t reads = 0, writes = 0; std::vector<uint8_t> out; };

static Run table_block(const Split& sp, uint32_t nlit_claimed, uint32_t isize, uint32_t ph, uint32_t T, Order order)
{
    Run r;
    if (isize == 0) return r;
    if (isize > MAX_OUT) { r.status = HANDOVER; return r; }
    // the stream: headers and literals in heap blocks of exactly their size (literal j at lit_end[-1 - j])
    const uint32_t nseq = (uint32_t)sp.hdr.size();
    uint32_t* hdr = static_cast<uint32_t*>(malloc(4u * nseq + (nseq ? 0 : 4)));
    if (nseq) memcpy(hdr, sp.hdr.data(), 4u * nseq);
    uint8_t* lits = static_cast<uint8_t*>(malloc(sp.lit.size() + (sp.lit.empty() ? 1 : 0)));
    for (size_t j = 0; j < sp.lit.size(); ++j) lits[sp.lit.size() - 1 - j] = sp.lit[j];
    const uint8_t* lit_end = lits + sp.lit.size();
    const uint32_t entries = round16(ph + isize);
    uint16_t* tab = static_cast<uint16_t*>(aligned_alloc(16, 2u * entries));
    for (uint32_t i = 0; i < entries; ++i) tab[i] = (uint16_t)(MAX_OUT - 1);           // an entry the build misses points far outside
    for (uint32_t t = 0; t < 32 && t < T; ++t) pad_write(tab, ph, isize, t);
    // build
    uint32_t W = 0, L = 0;
    std::vector<Seq> s(T);
    std::vector<uint32_t> w(T), l(T);
    for (uint32_t s0 = 0; s0 < nseq && r.status == LZ_OK; s0 += T) {
        uint32_t Tt = 0, Lt = 0;
        for (uint32_t t = 0; t < T; ++t) {
            s[t] = unpack(s0 + t < nseq ? hdr[s0 + t] : 0u);
            w[t] = W + Tt; l[t] = L + Lt;
            Tt += s[t].nl + s[t].ml; Lt += s[t].nl;
        }
        r.status = batch_check(W, Tt, isize, L, Lt, nlit_claimed);
        for (uint32_t t = 0; t < T && r.status == LZ_OK; ++t) r.status = seq_check(s[t], w[t]);
        if (r.status != LZ_OK) break;
        for (uint32_t k = 0; k < T; ++k) { const uint32_t t = order == REVERSE ? T - 1 - k : k; seq_write(tab, ph, s[t], w[t], lit_end, l[t]); }
        W += Tt; L += Lt;
    }
    if (r.status == LZ_OK && W != isize) r.status = LZ_SHORT;
    // resolve
    if (r.status == LZ_OK) {
        const uint32_t nw = n_words(ph, isize);
        std::vector<uint64_t> nxt(T);
        std::vector<uint8_t> chg(T);
        bool done = false;
        for (; r.rounds < MAX_ROUNDS && !done; ) {
            bool pending = false;
            for (uint32_t q0 = 0; q0 < nw; q0 += T) {
                const uint32_t nt = nw - q0 < T ? nw - q0 : T;
                for (uint32_t k = 0; k < nt; ++k) {
                    const uint32_t t = order == REVERSE ? nt - 1 - k : k;
                    bool changed = false;
                    nxt[t] = resolve_word(tab, ph, q0 + t, &changed, &pending);
                    chg[t] = changed;
                    r.reads += 4;
                    if (order != LOCKSTEP && changed) { word_write(tab, q0 + t, nxt[t]); r.writes += 4; }
                }
                if (order == LOCKSTEP)
                    for (uint32_t t = 0; t < nt; ++t) if (chg[t]) { word_write(tab, q0 + t, nxt[t]); r.writes += 4; }
            }
            ++r.rounds;
            done = !pending;
        }
        if (!done) r.status = LZ_SHORT;
    }
    // emit: the block's bytes behind `ph` bytes of its neighbour
    if (r.status == LZ_OK) {
        uint8_t* exact = static_cast<uint8_t*>(malloc(ph + isize));                        // (16-byte aligned: the chunks' stores are)
        memset(exact, 0xA5, ph);
        for (uint32_t c = 0; c < n_chunks(ph, isize); ++c) emit_chunk(tab, ph, isize, c, exact, ph);
        for (uint32_t i = 0; i < ph; ++i) if (exact[i] != 0xA5) r.status = -1;
        r.out.assign(exact + ph, exact + ph + isize);
        free(exact);
    }
    free(tab); free(lits); free(hdr);
    return r;
}

// ---- 3. drivers
static int g_failed = 0;
static void fail(const std::string& what) { printf("FAILED %s\n", what.c_str()); ++g_failed; }

static bool zlib_inflate(const uint8_t* src, size_t n, std::vector<uint8_t>& out)
{
    z_stream z; memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return false;
    out.resize(70000);
    z.next_in = const_cast<uint8_t*>(src); z.avail_in = (uInt)n;
    z.next_out = out.data(); z.avail_out = (uInt)out.size();
    const int rc = inflate(&z, Z_FINISH);
    out.resize(z.total_out);
    inflateEnd(&z);
    return rc == Z_STREAM_END;
}

struct Totals { long blocks = 0, skipped = 0, handed = 0; uint32_t max_rounds = 0; uint64_t rounds = 0, bytes = 0, reads = 0, writes = 0, seqs = 0, lits = 0; };

// ---- counting mode: the turns of the build's write loops, by the sequence streams alone (nothing is written).  A turn = one
// trip of a wave through a write loop, whatever the number of its lanes that are active in it.  Per batch of T sequences the
// build lasts as long as its slowest wave (the others wait at the barrier), so a block's turns are the sum over its batches of
// the largest value over the batch's waves of
//   by owner (every part by its sequence's thread: the kernel)   longest literal part + longest match part in the wave
//   LONG_RUN = R (parts of R entries or more by the whole wave,  longest literal part < R + longest match part < R in the wave
//   64 entries a turn: counted, built, measured slower and not   + the sum over the wave's parts >= R of ceil(entries / 64)
//   taken -- profiles/lz_table_build.txt)
static const uint32_t THRESHOLDS[3] = {16, 32, 64}, WAVE = 64;
struct Turns { uint64_t seqs = 0, bytes = 0, owner = 0, owner_lit = 0, owner_match = 0, scheme[3] = {0, 0, 0}, long_parts[3] = {0, 0, 0}, long_bytes[3] = {0, 0, 0}; };

static Turns count_block(const Split& sp, uint32_t T)
{
    Turns c;
    const uint32_t nseq = (uint32_t)sp.hdr.size();
    c.seqs = nseq;
    for (uint32_t s0 = 0; s0 < nseq; s0 += T) {
        uint64_t worst_owner = 0, worst_lit = 0, worst_match = 0, worst[3] = {0, 0, 0};
        for (uint32_t t0 = 0; t0 < T && s0 + t0 < nseq; t0 += WAVE) {
            uint32_t max_nl = 0, max_ml = 0, short_nl[3] = {0, 0, 0}, short_ml[3] = {0, 0, 0};
            uint64_t coop[3] = {0, 0, 0};
            for (uint32_t t = t0; t < t0 + WAVE && s0 + t < nseq; ++t) {
                const Seq s = unpack(sp.hdr[s0 + t]);
                c.bytes += s.nl + s.ml;
                if (s.nl > max_nl) max_nl = s.nl;
                if (s.ml > max_ml) max_ml = s.ml;
                for (int i = 0; i < 3; ++i) {
                    if (s.nl >= THRESHOLDS[i]) { coop[i] += (s.nl + WAVE - 1) / WAVE; ++c.long_parts[i]; c.long_bytes[i] += s.nl; }
                    else if (s.nl > short_nl[i]) short_nl[i] = s.nl;
                    if (s.ml >= THRESHOLDS[i]) { coop[i] += (s.ml + WAVE - 1) / WAVE; ++c.long_parts[i]; c.long_bytes[i] += s.ml; }
                    else if (s.ml > short_ml[i]) short_ml[i] = s.ml;
                }
            }
            if ((uint64_t)max_nl + max_ml > worst_owner) { worst_owner = (uint64_t)max_nl + max_ml; worst_lit = max_nl; worst_match = max_ml; }
            for (int i = 0; i < 3; ++i) { const uint64_t v = short_nl[i] + short_ml[i] + coop[i]; if (v > worst[i]) worst[i] = v; }
        }
        c.owner += worst_owner; c.owner_lit += worst_lit; c.owner_match += worst_match;
        for (int i = 0; i < 3; ++i) c.scheme[i] += worst[i];
    }
    return c;
}

static void add(Turns& a, const Turns& b)
{
    a.seqs += b.seqs; a.bytes += b.bytes; a.owner += b.owner; a.owner_lit += b.owner_lit; a.owner_match += b.owner_match;
    for (int i = 0; i < 3; ++i) { a.scheme[i] += b.scheme[i]; a.long_parts[i] += b.long_parts[i]; a.long_bytes[i] += b.long_bytes[i]; }
}

static void print_turns(const char* what, const Turns& c)
{
    printf("%s: sequences %llu, bytes %llu, turns by owner %llu (literals %llu + matches %llu)", what, (unsigned long long)c.seqs, (unsigned long long)c.bytes,
           (unsigned long long)c.owner, (unsigned long long)c.owner_lit, (unsigned long long)c.owner_match);
    for (int i = 0; i < 3; ++i)
        printf("; LONG_RUN %u: turns %llu, long parts %llu, long bytes %llu", THRESHOLDS[i], (unsigned long long)c.scheme[i], (unsigned long long)c.long_parts[i],
               (unsigned long long)c.long_bytes[i]);
    printf("\n");
}

static bool g_count = false;                             // --count: the build's turns per block and per file, nothing else

static void run_file(const char* path, Totals& tot)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fail(std::string(path) + ": cannot open"); return; }
    std::vector<uint8_t> raw;
    uint8_t tmp[1 << 16];
    for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) raw.insert(raw.end(), tmp, tmp + k);
    fclose(f);
    Totals t;
    Turns turns;
    size_t p = 0;
    long index = 0;
    while (p + 18 <= raw.size()) {
        if (!(raw[p] == 0x1f && raw[p + 1] == 0x8b && raw[p + 2] == 8 && (raw[p + 3] & 4))) { fail(std::string(path) + ": not a BGZF block"); break; }
        const size_t xlen = raw[p + 10] | raw[p + 11] << 8;
        size_t q = p + 12, bsize = 0;
        while (q + 4 <= p + 12 + xlen) {
            const size_t slen = raw[q + 2] | raw[q + 3] << 8;
            if (raw[q] == 66 && raw[q + 1] == 67) bsize = raw[q + 4] | raw[q + 5] << 8;
            q += 4 + slen;
        }
        if (!bsize || p + bsize + 1 > raw.size()) break;
        const size_t end = p + bsize + 1, at = p + 12 + xlen, n = end - 8 - at;
        uint32_t isize; memcpy(&isize, &raw[end - 4], 4);
        p = end;
        ++index;
        std::vector<uint8_t> want;
        if (!zlib_inflate(&raw[at], n, want) || want.size() != isize) { ++t.skipped; continue; }       // malformed: the tokens kernel's business
        Split sp;
        if (!deflate_to_split(&raw[at], n, sp)) { fail(std::string(path) + ": the parser refuses a block zlib takes"); continue; }
        if (g_count) {
            if (isize > MAX_OUT) { ++t.handed; continue; }
            const Turns c = count_block(sp, 1024);
            print_turns((std::string(path) + " block " + std::to_string(index - 1)).c_str(), c);
            add(turns, c);
            ++t.blocks;
            continue;
        }
        const uint32_t ph = (uint32_t)(index * 7 + 3) & 15u;
        const struct { uint32_t T; Order o; } modes[] = {{1024, LOCKSTEP}, {1024, REVERSE}, {512, FORWARD}};
        for (const auto& m : modes) {
            const Run r = table_block(sp, (uint32_t)sp.lit.size(), isize, ph, m.T, m.o);
            if (isize > MAX_OUT) { if (r.status != HANDOVER) fail(std::string(path) + ": a block above 0xFF00 bytes was not refused"); continue; }
            if (r.status != LZ_OK || r.out != want) { fail(std::string(path) + ": block " + std::to_string(index - 1) + " status " + std::to_string(r.status) + (r.out != want ? ", bytes differ" : "")); break; }
            if (m.o == LOCKSTEP) { t.rounds += r.rounds; t.reads += r.reads; t.writes += r.writes; if (r.rounds > t.max_rounds) t.max_rounds = r.rounds; }
        }
        if (isize > MAX_OUT) { ++t.handed; continue; }
        ++t.blocks; t.bytes += isize; t.seqs += sp.hdr.size(); t.lits += sp.lit.size();
    }
    if (g_count) {
        printf("%s: counted  blocks %ld (+ %ld malformed skipped, %ld above 0xFF00 handed over)\n", path, t.blocks, t.skipped, t.handed);
        print_turns((std::string(path) + " in all").c_str(), turns);
        tot.blocks += t.blocks;
        return;
    }
    printf("%s: ok  blocks %ld (+ %ld malformed skipped, %ld above 0xFF00 handed over), sequences/block %.0f, literal bytes %.1f %%, rounds mean %.2f max %u, "
           "table reads/byte %.1f writes/byte %.2f\n", path, t.blocks, t.skipped, t.handed, t.blocks ? (double)t.seqs / t.blocks : 0.0,
           t.bytes ? 100.0 * t.lits / t.bytes : 0.0, t.blocks ? (double)t.rounds / t.blocks : 0.0, t.max_rounds,
           t.bytes ? (double)t.reads / t.bytes : 0.0, t.bytes ? (double)t.writes / t.bytes : 0.0);
    tot.blocks += t.blocks;
}

static uint32_t H(uint32_t nl, uint32_t ml, uint32_t d) { return nl | ml << 8 | (d - 1u) << 17; }

static void crafted()
{
    struct Case { const char* name; Split sp; uint32_t isize; int want_status; std::vector<uint8_t> want; int nlit_delta; };
    std::vector<Case> cases;
    {   // 1 literal + 65,279 copies at distance 1: the deepest chain a block can hold, ISIZE exactly 0xFF00
        Case c{"run_distance1_0xFF00", {}, MAX_OUT, LZ_OK, std::vector<uint8_t>(MAX_OUT, 'x'), 0};
        c.sp.lit.push_back('x');
        uint32_t left = MAX_OUT - 1;
        c.sp.hdr.push_back(H(1, 258, 1)); left -= 258;
        while (left) { const uint32_t m = left < 258 ? left : 258; c.sp.hdr.push_back(H(0, m, 1)); left -= m; }
        cases.push_back(c);
        Case d = c; d.name = "isize_0xFF01_refused"; d.isize = MAX_OUT + 1; d.sp.hdr.push_back(H(0, 1, 1)); d.want_status = HANDOVER; d.want.clear();
        cases.push_back(d);
    }
    cases.push_back(Case{"empty", {}, 0, LZ_OK, {}, 0});
    {   // stored only: literal-only sequences of 255
        Case c{"stored_only", {}, 1000, LZ_OK, {}, 0};
        for (uint32_t i = 0; i < 1000; ++i) { c.sp.lit.push_back((uint8_t)(i * 37)); c.want.push_back((uint8_t)(i * 37)); }
        for (uint32_t left = 1000; left; ) { const uint32_t n = left < 255 ? left : 255; c.sp.hdr.push_back(n); left -= n; }
        cases.push_back(c);
    }
    {   // a match that reaches the block's first byte, overlapping itself; one a byte further is flagged
        Case c{"match_to_first_byte", {}, 8, LZ_OK, {'a', 'b', 'c', 'a', 'b', 'c', 'a', 'b'}, 0};
        c.sp.lit = {'a', 'b', 'c'}; c.sp.hdr = {H(3, 5, 3)};
        cases.push_back(c);
        Case d = c; d.name = "distance_past_the_start"; d.sp.hdr = {H(3, 5, 4)}; d.want_status = LZ_BAD_DIST; d.want.clear();
        cases.push_back(d);
        Case f = c; f.name = "long_match_past_the_start"; f.sp.hdr = {H(3, 258, 4)}; f.isize = 261; f.want_status = LZ_BAD_DIST; f.want.clear();
        cases.push_back(f);
        Case e = c; e.name = "distance_past_the_start_second_batch"; e.sp.hdr.clear(); e.sp.lit.clear();
        for (uint32_t i = 0; i < 1500; ++i) { e.sp.hdr.push_back(H(1, 0, 1)); e.sp.lit.push_back('q'); }
        e.sp.hdr.push_back(H(0, 4, 1501)); e.isize = 1504; e.want_status = LZ_BAD_DIST; e.want.clear();
        cases.push_back(e);
    }
    {   // sums that overrun ISIZE / the literals the stream holds / a stream that stops short
        Case c{"output_overrun", {}, 7, LZ_OUT_OVERRUN, {}, 0};
        c.sp.lit = {'a', 'b', 'c'}; c.sp.hdr = {H(3, 5, 3)};
        cases.push_back(c);
        Case d = c; d.name = "literal_overrun"; d.isize = 8; d.nlit_delta = -1;
        cases.push_back(d);
        Case e = c; e.name = "short_stream"; e.isize = 9; e.want_status = LZ_SHORT;
        cases.push_back(e);
    }
    for (const Case& c : cases)
        for (uint32_t ph : {0u, 1u, 9u, 15u})
            for (int o = 0; o < 3; ++o)
                for (uint32_t T : {1024u, 512u, 64u}) {
                    const Run r = table_block(c.sp, (uint32_t)((int)c.sp.lit.size() + c.nlit_delta), c.isize, ph, T, (Order)o);
                    if (r.status != c.want_status || (c.want_status == LZ_OK && r.out != c.want)) fail(std::string("crafted ") + c.name + ": status " + std::to_string(r.status));
                    if (r.rounds > MAX_ROUNDS) fail(std::string("crafted ") + c.name + ": rounds");
                    if (ph == 0 && o == 0 && T == 1024) printf("crafted %s: status %d, rounds %u\n", c.name, r.status, r.rounds);
                }
    printf("crafted: ok\n");
}

int main(int argc, char** argv)
{
    g_count = argc > 1 && std::string(argv[1]) == "--count";
    const int first = g_count ? 2 : 1;
    if (!g_count) crafted();
    Totals tot;
    for (int i = first; i < argc; ++i) run_file(argv[i], tot);
    printf("%ld blocks in %d files, %d failures\n", tot.blocks, argc - first, g_failed);
    return g_failed ? 1 : 0;
}
