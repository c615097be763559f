// svx_recsort_core.hpp -- a lane's share of scatter_segments_kernel and of record_retid_kernel (svx_recsort.hip), host- and
// device-compilable: the host programs tools/hostwave/scatter_main.cpp and retid_main.cpp run this very code, lane by lane, under
// AddressSanitizer.
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

}  // namespace svx_recsort
