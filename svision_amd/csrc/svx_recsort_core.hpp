// svx_recsort_core.hpp -- a lane's share of scatter_segments_kernel, of record_retid_kernel, of the two record_retag kernels and of
// the two record_tags kernels (svx_recsort.hip), host- and device-compilable: the host programs tools/hostwave/scatter_main.cpp,
// retid_main.cpp, retag_main.cpp and tags_main.cpp run this very code, lane by lane, under AddressSanitizer.
//
// A wave of 64 lanes copies one segment.  The DESTINATION decides the alignment, as in gather_segments_kernel: single bytes up to
// its first dword boundary, whole dwords -- each assembled from the one or two aligned source dwords that hold its bytes --,
// single bytes behind the last whole dword.  The source is read only in the aligned dwords that hold the segment's own bytes: the
// array it lies in is 4-byte aligned and readable up to the next multiple of 4 behind its last byte.  Nothing outside
// to[0 .. len) is written.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SVX_RS_HD __host__ __device__ __forceinline__
#else
#define SVX_RS_HD inline
#endif

namespace svx_recsort {

constexpr uint32_t WAVE = 64;

// Lane `lane` of the wave that copies from[0 .. len) to to[0 .. len).
SVX_RS_HD void copy_segment(const uint8_t* from, uint8_t* to, uint64_t len, uint32_t lane)
{
    uint64_t head = (uint64_t)(-reinterpret_cast<uintptr_t>(to) & 3u);
    if (head > len) head = len;
    if (lane < head) to[lane] = from[lane];
    const uint64_t words = (len - head) / 4;
    const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(from + head) & 3u), shift = skew * 8;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(from + head - skew);
    uint32_t* out = reinterpret_cast<uint32_t*>(to + head);
    for (uint64_t j = lane; j < words; j += WAVE) {
        uint32_t v = in[j];
        if (shift) v = v >> shift | in[j + 1] << (32 - shift);  // (in[j + 1] holds the word's last byte: inside the segment's dwords)
        out[j] = v;
    }
    const uint64_t done = head + words * 4;
    if (done + lane < len) to[done + lane] = from[done + lane];
}

// Lane `lane` of the wave of INPUT record i: where the record's rank lies in [rank_lo, rank_hi), its bytes
// src[src_off[i] .. src_off[i + 1]) go to dst + off_out[rank] - out_base.  A record whose length is not the one the output's
// offsets give it (off_out[rank + 1] - off_out[rank]) is not copied: *status = 1, a plain store of one value.
SVX_RS_HD void scatter_record(const uint8_t* src, const int64_t* src_off, const uint32_t* rank, uint32_t rank_lo, uint32_t rank_hi,
                              const int64_t* off_out, int64_t out_base, uint8_t* dst, uint64_t i, uint32_t lane, int32_t* status)
{
    const uint32_t r = rank[i];
    if (r < rank_lo || r >= rank_hi) return;                    // (the same answer in every lane: whole waves leave)
    const int64_t len = src_off[i + 1] - src_off[i];
    if (len != off_out[(uint64_t)r + 1] - off_out[r]) {
        if (lane == 0) *status = 1;
        return;
    }
    copy_segment(src + src_off[i], dst + (off_out[r] - out_base), (uint64_t)len, lane);
}

// ---- record_retid_kernel's share of one record (tools/hostwave/retid_main.cpp runs it under AddressSanitizer) ----
// A BAM record's two reference indices are little-endian int32 at bytes 4 (refID) and 24 (next_refID) behind its block_size field.
// Records start at any byte offset, so the fields are read and written byte by byte: no access leaves bytes 4..7 and 24..27.
SVX_RS_HD int32_t load_le32(const uint8_t* p)
{
    return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}

SVX_RS_HD void store_le32(uint8_t* p, int32_t value)
{
    const uint32_t v = (uint32_t)value;
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// -1 stays -1, 0 <= v < n_in becomes map[v] -> true; anything else: false, *out untouched.
SVX_RS_HD bool retid_value(int32_t v, const int32_t* map, int32_t n_in, int32_t* out)
{
    if (v == -1) { *out = -1; return true; }
    if (v < 0 || v >= n_in) return false;
    *out = map[v];
    return true;
}

// The lane of record r: both fields through `map`, and tid_key[r] where it is given.  A field outside [-1, n_in) leaves BOTH
// fields of the record as they are and sets *status (a plain store of the one value); a key outside likewise stays.
SVX_RS_HD void retid_record(uint8_t* bytes, const int64_t* off, const int32_t* map, int32_t n_in, int32_t* tid_key, uint64_t r,
                            int32_t* status)
{
    uint8_t* rec = bytes + off[r];
    const int32_t tid = load_le32(rec + 4), next = load_le32(rec + 24);
    int32_t new_tid, new_next;
    if (retid_value(tid, map, n_in, &new_tid) && retid_value(next, map, n_in, &new_next)) {
        if (new_tid != tid) store_le32(rec + 4, new_tid);
        if (new_next != next) store_le32(rec + 24, new_next);
    } else {
        *status = 1;
    }
    if (tid_key) {
        int32_t key;
        if (retid_value(tid_key[r], map, n_in, &key)) tid_key[r] = key;
        else *status = 1;
    }
}

// ---- record_retag_measure_kernel's and record_retag_write_kernel's share of one record (tools/hostwave/retag_main.cpp) ----
// A WAVE per record.  The optional fields behind qual are a chain: every lane follows it with the same loads and takes the same
// turns; only the search for the NUL of a Z / H value is shared out, 64 bytes a step, and only the copies of retag_write.
//
// The table: m entries, entry e = a 2-byte tag, an old value and a new one, packed in `bytes` with 2m + 1 offsets:
// tag = bytes[off[2e]], bytes[off[2e] + 1]; old = bytes[off[2e] + 2 .. off[2e + 1]); new = bytes[off[2e + 1] .. off[2e + 2]).
// Values carry no NUL.  Only the tags RG and PG are looked for.
struct RetagTable {
    const uint8_t* bytes;
    const int32_t* off;
    int32_t m;
};

// What a record needs: `n` replacements (0 .. 2) in the order they lie in the record -- the value at bytes [at, at + old_len) of
// the record becomes table entry `entry`'s new value --, the record's new length, and whether the record is malformed (then n = 0
// and new_len is the old length).  The same in every lane.
struct RetagPlan {
    uint32_t n;
    uint64_t at[2], old_len[2];
    int32_t entry[2];
    uint64_t new_len;
    bool bad;
};

// The bits of the lanes l < count whose byte p[l] is 0 (count <= 64); on the host a loop over the lanes.
SVX_RS_HD uint64_t ballot_nul(const uint8_t* p, uint64_t count, uint32_t lane)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(lane < count && p[lane] == 0);
#else
    (void)lane;
    uint64_t mask = 0;
    for (uint32_t l = 0; l < WAVE; ++l)
        if (l < count && p[l] == 0) mask |= 1ull << l;
    return mask;
#endif
}

SVX_RS_HD uint32_t lowest_bit(uint64_t mask)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__ffsll((unsigned long long)mask) - 1u;
#else
    uint32_t b = 0;
    while (!(mask & 1)) { mask >>= 1; ++b; }
    return b;
#endif
}

// 1, 2, 4: the bytes of a value of type t (A c C, s S, i I f); 0: no fixed-size type.
SVX_RS_HD uint32_t retag_fixed_size(uint8_t t)
{
    if (t == 'A' || t == 'c' || t == 'C') return 1;
    if (t == 's' || t == 'S') return 2;
    if (t == 'i' || t == 'I' || t == 'f') return 4;
    return 0;
}

// The entry whose tag is (t0, t1) and whose old value is value[0 .. len), or -1.
SVX_RS_HD int32_t retag_lookup(const RetagTable& tb, uint8_t t0, uint8_t t1, const uint8_t* value, uint64_t len)
{
    for (int32_t e = 0; e < tb.m; ++e) {
        const uint8_t* ent = tb.bytes + tb.off[2 * e];
        if (ent[0] != t0 || ent[1] != t1 || (uint64_t)(tb.off[2 * e + 1] - tb.off[2 * e] - 2) != len) continue;
        uint64_t k = 0;
        while (k < len && ent[2 + k] == value[k]) ++k;
        if (k == len) return e;
    }
    return -1;
}

// Where the optional fields of the record rec[0 .. len) begin, behind qual; 0: shorter than 36 bytes, block_size + 4 != len, or the
// fixed part with name, CIGAR, seq and qual longer than the record.  Byte loads inside the record.
SVX_RS_HD uint64_t aux_start(const uint8_t* rec, int64_t len)
{
    if (len < 36 || (int64_t)load_le32(rec) + 4 != len) return 0;
    const uint64_t l_name = rec[12], n_cigar = (uint64_t)rec[16] | (uint64_t)rec[17] << 8, l_seq = (uint32_t)load_le32(rec + 20);
    const uint64_t p = 36 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
    return p > (uint64_t)len ? 0 : p;
}

// One step of the chain: the field that begins at rec[p], p < end, of a record that ends at rec[end] -> the offset behind it, 0: a
// field header cut by the end, an unknown type or B subtype, a value or a B array past the end, a Z / H without NUL (whose NUL,
// where there is one, is the byte in front of the offset returned).  The same loads and the same answer in every lane; the lanes
// share only the search for the NUL, 64 bytes a ballot.  A B array is skipped in one step from its count.
SVX_RS_HD uint64_t field_next(const uint8_t* rec, uint64_t p, uint64_t end, uint32_t lane)
{
    if (p + 3 > end) return 0;
    const uint8_t type = rec[p + 2];
    const uint64_t v = p + 3;
    const uint32_t fixed = retag_fixed_size(type);
    if (fixed) return v + fixed > end ? 0 : v + fixed;
    if (type == 'Z' || type == 'H') {
        for (uint64_t q = v; q < end; q += WAVE) {              // 64 bytes a step: the lowest lane that holds a NUL
            const uint64_t mask = ballot_nul(rec + q, end - q < WAVE ? end - q : WAVE, lane);
            if (mask) return q + lowest_bit(mask) + 1;
        }
        return 0;
    }
    if (type != 'B' || v + 5 > end) return 0;
    const uint32_t elem = retag_fixed_size(rec[v]);
    if (!elem || rec[v] == 'A') return 0;
    const uint64_t count = (uint32_t)load_le32(rec + v + 1);
    return count * elem > end - (v + 5) ? 0 : v + 5 + count * elem;
}

// The plan of the record rec[0 .. len): nothing outside those bytes is read, byte by byte.  Malformed: what aux_start and
// field_next refuse.
SVX_RS_HD RetagPlan retag_plan(const uint8_t* rec, int64_t len, const RetagTable& tb, uint32_t lane)
{
    RetagPlan plan;
    plan.n = 0;
    plan.new_len = len < 0 ? 0 : (uint64_t)len;
    plan.bad = true;
    plan.at[0] = plan.at[1] = plan.old_len[0] = plan.old_len[1] = 0;
    plan.entry[0] = plan.entry[1] = -1;
    uint64_t p = aux_start(rec, len);
    if (!p) return plan;
    const uint64_t end = (uint64_t)len;
    bool done_rg = false, done_pg = false;
    uint32_t n = 0;
    int64_t grow = 0;
    while (p < end) {
        const uint64_t next = field_next(rec, p, end, lane);
        if (!next) return plan;
        const uint8_t t0 = rec[p], t1 = rec[p + 1];
        const bool rg = t0 == 'R' && t1 == 'G', pg = t0 == 'P' && t1 == 'G';
        if (rec[p + 2] == 'Z' && ((rg && !done_rg) || (pg && !done_pg))) {
            const uint64_t v = p + 3, nul = next - 1;
            const int32_t e = retag_lookup(tb, t0, t1, rec + v, nul - v);
            if (e >= 0) {
                plan.at[n] = v; plan.old_len[n] = nul - v; plan.entry[n] = e;
                grow += (int64_t)(tb.off[2 * e + 2] - tb.off[2 * e + 1]) - (int64_t)(nul - v);
                ++n;
                if (rg) done_rg = true; else done_pg = true;
            }
        }
        p = next;
    }
    plan.n = n;
    plan.new_len = (uint64_t)((int64_t)end + grow);
    plan.bad = false;
    return plan;
}

// Lane `lane` of the wave of record r, measure: new_len[r] = the record's length with its values replaced; a malformed record keeps
// its length and sets *status (a plain store of the one value).
SVX_RS_HD void retag_measure_record(const uint8_t* bytes, const int64_t* off, const RetagTable& tb, int64_t* new_len, uint64_t r, uint32_t lane,
                                    int32_t* status)
{
    const RetagPlan plan = retag_plan(bytes + off[r], off[r + 1] - off[r], tb, lane);
    if (lane == 0) {
        new_len[r] = (int64_t)plan.new_len;
        if (plan.bad) *status = 1;
    }
}

// Lane `lane` of the wave of record r, write: the record with its values replaced and its block_size set goes to
// dst[new_off[r] .. new_off[r + 1]), in up to five pieces (copy_segment: any skew of source and destination); a malformed record
// is copied as it is and sets *status.  Where new_off does not give the record the length of its plan, nothing is written and
// *status is set.  The table's bytes are read like a record's: in the aligned dwords that hold a value.
SVX_RS_HD void retag_write_record(const uint8_t* bytes, const int64_t* off, const RetagTable& tb, const int64_t* new_off, uint8_t* dst, uint64_t r,
                                  uint32_t lane, int32_t* status)
{
    const uint8_t* rec = bytes + off[r];
    const int64_t len = off[r + 1] - off[r];
    const RetagPlan plan = retag_plan(rec, len, tb, lane);
    if (plan.bad && lane == 0) *status = 1;
    if (new_off[r + 1] - new_off[r] != (int64_t)plan.new_len) {
        if (lane == 0) *status = 1;
        return;
    }
    uint8_t* out = dst + new_off[r];
    if (plan.n == 0) {
        copy_segment(rec, out, plan.new_len, lane);
        return;
    }
    if (lane < 4) out[lane] = (uint8_t)((uint32_t)(plan.new_len - 4) >> (8 * lane));        // block_size
    uint64_t from = 4, to = 4;
    for (uint32_t k = 0; k < plan.n; ++k) {
        const int32_t e = plan.entry[k];
        const uint64_t value_len = (uint64_t)(tb.off[2 * e + 2] - tb.off[2 * e + 1]);
        copy_segment(rec + from, out + to, plan.at[k] - from, lane);
        to += plan.at[k] - from;
        copy_segment(tb.bytes + tb.off[2 * e + 1], out + to, value_len, lane);
        to += value_len;
        from = plan.at[k] + plan.old_len[k];
    }
    copy_segment(rec + from, out + to, (uint64_t)len - from, lane);
}

// ---- record_tags_measure_kernel's and record_tags_write_kernel's share of one record (tools/hostwave/tags_main.cpp) ----
// Optional fields removed by their tag.  A WAVE per record, the chain followed as above (aux_start, field_next).  The table is a
// bitmap over ALL 65,536 two-byte values, 2,048 dwords: bit (t0 | t1 << 8) set = a field of the tag (t0, t1) is REMOVED.  One
// dword load and a shift a field, the same in every lane, whatever bytes a record's tags hold; a keep list is the complement, made
// on the host, so the kernels know one rule.
constexpr uint32_t TAGS_TABLE_WORDS = 2048;

SVX_RS_HD bool tags_removed(const uint32_t* table, uint8_t t0, uint8_t t1)
{
    const uint32_t k = (uint32_t)t0 | (uint32_t)t1 << 8;
    return (table[k >> 5] >> (k & 31u)) & 1u;
}

// The length of the record rec[0 .. len) without the fields that `table` removes; *bad: malformed (what aux_start and field_next
// refuse; the length is then the record's own).  Byte loads inside the record.  The same in every lane.
SVX_RS_HD uint64_t tags_new_len(const uint8_t* rec, int64_t len, const uint32_t* table, uint32_t lane, bool* bad)
{
    const uint64_t end = len < 0 ? 0 : (uint64_t)len;
    *bad = true;
    uint64_t p = aux_start(rec, len), removed = 0;
    if (!p) return end;
    while (p < end) {
        const uint64_t next = field_next(rec, p, end, lane);
        if (!next) return end;
        if (tags_removed(table, rec[p], rec[p + 1])) removed += next - p;
        p = next;
    }
    *bad = false;
    return end - removed;
}

// Lane `lane` of the wave of record r, measure: new_len[r] = the record's length without the removed fields; a malformed record
// keeps its length and sets *status (a plain store of the one value).
SVX_RS_HD void tags_measure_record(const uint8_t* bytes, const int64_t* off, const uint32_t* table, int64_t* new_len, uint64_t r, uint32_t lane,
                                   int32_t* status)
{
    bool bad;
    const uint64_t n = tags_new_len(bytes + off[r], off[r + 1] - off[r], table, lane, &bad);
    if (lane == 0) {
        new_len[r] = (int64_t)n;
        if (bad) *status = 1;
    }
}

// Lane `lane` of the wave of record r, write: the record without the removed fields and with its block_size set goes to
// dst[new_off[r] .. new_off[r + 1]).  The chain is walked for the length first: where new_off does not give the record that
// length, nothing is written and *status is set.  Then it is walked again, and the fixed part with the fields up to the first
// removed one, and every further maximal run of kept fields, is ONE copy_segment (any skew of source and destination) -- the
// removed fields have no bound, so no plan holds them; the walk is the plan.  A malformed record is copied as it is and sets *status,
// a record that loses nothing is one copy.
SVX_RS_HD void tags_write_record(const uint8_t* bytes, const int64_t* off, const uint32_t* table, const int64_t* new_off, uint8_t* dst, uint64_t r,
                                 uint32_t lane, int32_t* status)
{
    const uint8_t* rec = bytes + off[r];
    const int64_t len = off[r + 1] - off[r];
    bool bad;
    const uint64_t new_len = tags_new_len(rec, len, table, lane, &bad);
    if (bad && lane == 0) *status = 1;
    if (new_off[r + 1] - new_off[r] != (int64_t)new_len) {
        if (lane == 0) *status = 1;
        return;
    }
    uint8_t* out = dst + new_off[r];
    const uint64_t end = (uint64_t)len;
    if (bad || new_len == end) {
        copy_segment(rec, out, new_len, lane);
        return;
    }
    if (lane < 4) out[lane] = (uint8_t)((uint32_t)(new_len - 4) >> (8 * lane));             // block_size
    uint64_t from = 4, to = 4, p = aux_start(rec, len);        // rec[from .. p): the run of kept bytes that is open
    while (p < end) {
        const uint64_t next = field_next(rec, p, end, lane);
        if (!next) return;                                      // (not reached: the first walk went through the same bytes)
        if (tags_removed(table, rec[p], rec[p + 1])) {
            if (p > from) copy_segment(rec + from, out + to, p - from, lane);
            to += p - from;
            from = next;
        }
        p = next;
    }
    if (end > from) copy_segment(rec + from, out + to, end - from, lane);
}

}  // namespace svx_recsort
