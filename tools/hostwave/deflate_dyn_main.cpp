// deflate_dyn_main.cpp -- bgzf_deflate_dyn_kernel (svision_amd/csrc/svx_deflate.hip) without a GPU: svx_dfl::encode_block_dyn of
// svx_deflate_core.hpp -- the code the kernel runs -- with the workgroup's threads as loops.
//
// As deflate_main.cpp: a phase (each) is T threads between two barriers, run FORWARD, in REVERSE or STRIDED (the odd threads before
// the even ones); the racing accesses are the table inserts (atomic max), the chain marks, the histogram and size sums (atomic add)
// and the bit writes (atomic or), so the three orders must give the same member, byte for byte.
// Built with -fsanitize=address,undefined: the block, every LDS array, the block's workspace (token bytes of n, mark words of
// (n + 31) / 32) and the member (n + 31 bytes) live in heap blocks of exactly their size.  On the device the code construction's
// arrays and the staging area share the hash table's LDS; here they are blocks of their own, filled with 0xA5 like the rest.
// The CRC32 in the footer is zlib's here; on the device svx_crc.hip writes it.
//
// usage: deflate_dyn_host CASES OUT [ORDERS]   CASES: u32 n, u64 off[n + 1], the stream's bytes (block b = bytes off[b] .. off[b + 1])
//                                               OUT.0 / OUT.1 / OUT.2 (one per order, the first ORDERS of them, default all three):
//                                               u32 n, u32 len[n], u32 btype[n], the members end to end
#include <zlib.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../svision_amd/csrc/svx_deflate_core.hpp"

using namespace svx_dfl;

enum Order { FORWARD = 0, REVERSE = 1, STRIDED = 2, ORDERS = 3 };

struct HostGroup {
    Order order;
    template <class F> void each(F f)
    {
        if (order == FORWARD) for (uint32_t t = 0; t < T; ++t) f(t);
        else if (order == REVERSE) for (uint32_t t = T; t-- > 0;) f(t);
        else { for (uint32_t t = 1; t < T; t += 2) f(t); for (uint32_t t = 0; t < T; t += 2) f(t); }
    }
    void barrier() {}
    void wave_sync() {}
    void tick(uint32_t) {}
    void atomic_max(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
    void atomic_or(uint32_t* p, uint32_t v) { *p |= v; }
    void atomic_add(uint32_t* p, uint32_t v) { *p += v; }
    void scan(uint32_t* a, uint32_t* total)
    {
        uint32_t run = 0;
        for (uint32_t t = 0; t < T; ++t) { const uint32_t v = a[t]; a[t] = run; run += v; }
        *total = run;
    }
};

// heap blocks of exactly their sizes, holding whatever the workgroup in front left there: an index one past any array is the
// sanitizer's to catch
struct HostLds {
    Ctx c;
    DynCtx d;
    std::vector<void*> blocks;
    template <class P> void get(P*& p, size_t bytes)
    {
        p = (P*)malloc(bytes ? bytes : 1);
        memset(p, 0xA5, bytes ? bytes : 1);
        blocks.push_back(p);
    }
    void huff(Huff& h, uint32_t n, uint32_t maxbits)
    {
        h.n = n; h.maxbits = maxbits;
        get(h.w, 4 * n); get(h.sw, 4 * n); get(h.nfreq, 4 * n); get(h.order, 2 * n); get(h.parent, 4 * n); get(h.len, n); get(h.code, 2 * n);
        get(h.st, 4 * ST_WORDS);
    }
    explicit HostLds(uint32_t n)
    {
        get(c.in, n); get(c.table, 4 * TABLE_ENTRIES); get(c.keys, 4 * T); get(c.cand, 4 * T); get(c.tokoff, 4 * T);
        get(c.stage, 4 * STAGE_WORDS); get(c.s, 16); get(c.mlen, 2 * T); get(c.mdist, 2 * T); get(c.nxt_a, 2 * T); get(c.nxt_b, 2 * T);
        get(c.mark, T);
        get(d.hist_lit, 4 * NLIT); get(d.hist_dist, 4 * NDIST);
        huff(d.lit, NLIT, CODE_BITS); huff(d.dist, NDIST, CODE_BITS); huff(d.cl, NCL_ROOM, CL_BITS);
        get(d.seq_sym, SEQ_ROOM); get(d.seq_ext, SEQ_ROOM); get(d.ds, 4 * D_WORDS); get(d.stage2, 4 * STAGE2_WORDS);
        get(d.ws_tok, n); get(d.ws_mark, 4 * ((n + 31) / 32));
    }
    ~HostLds() { for (void* p : blocks) free(p); }
};

int main(int argc, char** argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: deflate_dyn_host CASES OUT [ORDERS]\n"); return 2; }
    const int orders = argc == 4 ? atoi(argv[3]) : (int)ORDERS;
    if (orders < 1 || orders > (int)ORDERS) { fprintf(stderr, "ORDERS: 1 .. %d\n", (int)ORDERS); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    std::vector<uint64_t> off(n + 1);
    if (fread(off.data(), 8, n + 1, f) != n + 1) return 2;
    std::vector<uint8_t> stream(off[n]);
    if (off[n] && fread(stream.data(), 1, off[n], f) != off[n]) return 2;
    fclose(f);
    for (int o = 0; o < orders; ++o) {
        std::vector<uint32_t> lens(n), btype(n);
        std::vector<uint8_t> all;
        for (uint32_t b = 0; b < n; ++b) {
            const uint32_t len = (uint32_t)(off[b + 1] - off[b]);
            if (len > MAX_IN) { fprintf(stderr, "block %u: %u bytes\n", b, len); return 2; }
            uint8_t* src = (uint8_t*)malloc(len ? len : 1);
            memcpy(src, stream.data() + off[b], len);
            uint8_t* member = (uint8_t*)malloc(len + HEADER + STORED_EXTRA + FOOTER);
            memset(member, 0x5A, len + HEADER + STORED_EXTRA + FOOTER);
            {
                HostLds lds(len);
                HostGroup g{(Order)o};
                encode_block_dyn(g, lds.c, lds.d, src, len, member, &lens[b], &btype[b]);
                // the size the choice was made by is the size the bits phase wrote
                if (btype[b] != FORM_STORED && lds.d.ds[D_END] != lds.d.ds[D_PAYLOAD]) {
                    printf("FAILED block %u order %d: %u bytes counted, %u written\n", b, o, lds.d.ds[D_PAYLOAD], lds.d.ds[D_END]);
                    return 1;
                }
            }
            if (btype[b] > FORM_DYNAMIC || lens[b] < HEADER + FOOTER || lens[b] > len + HEADER + STORED_EXTRA + FOOTER) {
                printf("FAILED block %u order %d: member of %u bytes, type %u\n", b, o, lens[b], btype[b]);
                return 1;
            }
            const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, len);
            for (int k = 0; k < 4; ++k) member[lens[b] - 8 + k] = (uint8_t)(crc >> (8 * k));
            all.insert(all.end(), member, member + lens[b]);
            free(member); free(src);
        }
        const std::string path = std::string(argv[2]) + "." + std::to_string(o);
        FILE* out = fopen(path.c_str(), "wb");
        if (!out) { perror(path.c_str()); return 2; }
        fwrite(&n, 4, 1, out);
        if (n) { fwrite(lens.data(), 4, n, out); fwrite(btype.data(), 4, n, out); fwrite(all.data(), 1, all.size(), out); }
        fclose(out);
    }
    printf("deflate_dyn_host: ok, %u blocks, %d orders\n", n, orders);
    return 0;
}
