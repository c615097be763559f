// deflate_main.cpp -- bgzf_deflate_kernel (svision_amd/csrc/svx_deflate.hip) without a GPU: svx_dfl::encode_block of
// svx_deflate_core.hpp -- the code the kernel runs -- with the workgroup's threads as loops.
//
// A phase (each) is T threads between two barriers; the kernel's waves run it in any interleaving.  The racing accesses are the
// table inserts (atomic max), the chain marks (every writer stores 1) and the bit writes (atomic or), so three orders of the
// threads of a phase -- FORWARD first to last, REVERSE last to first, STRIDED the odd threads before the even ones -- must give
// the same member, byte for byte (the Python side compares the files and checks every member against zlib).
// Built with -fsanitize=address,undefined: the block, the workgroup's LDS image and the member live in heap blocks of exactly
// their size -- the member's of n + 31 bytes, the bound include/svx.h states (a slot on the device is 65,536).
// The CRC32 in the footer is zlib's here; on the device svx_crc.hip writes it.
//
// usage: deflate_host CASES OUT [ORDERS]   CASES: u32 n, u64 off[n + 1], the stream's bytes (block b = bytes off[b] .. off[b + 1])
//                                           OUT.0 / OUT.1 / OUT.2 (one per order, the first ORDERS of them, default all three):
//                                           u32 n, u32 len[n], u32 stored[n], the members end to end
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
    void atomic_max(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
    void atomic_or(uint32_t* p, uint32_t v) { *p |= v; }
    void scan(uint32_t* a, uint32_t* total)
    {
        uint32_t run = 0;
        for (uint32_t t = 0; t < T; ++t) { const uint32_t v = a[t]; a[t] = run; run += v; }
        *total = run;
    }
};

// the LDS image as separate heap blocks of exactly their sizes: an index one past any array is the sanitizer's to catch
struct HostLds {
    Ctx c;
    explicit HostLds(uint32_t n)
    {
        c.in = (uint8_t*)malloc(n ? n : 1);
        c.table = (uint32_t*)malloc(4 * TABLE_ENTRIES);
        c.keys = (uint32_t*)malloc(4 * T); c.cand = (uint32_t*)malloc(4 * T); c.tokoff = (uint32_t*)malloc(4 * T);
        c.stage = (uint32_t*)malloc(4 * STAGE_WORDS); c.s = (uint32_t*)malloc(16);
        c.mlen = (uint16_t*)malloc(2 * T); c.mdist = (uint16_t*)malloc(2 * T); c.nxt_a = (uint16_t*)malloc(2 * T); c.nxt_b = (uint16_t*)malloc(2 * T);
        c.mark = (uint8_t*)malloc(T);
        // (LDS holds whatever the workgroup in front left there)
        memset(c.table, 0xA5, 4 * TABLE_ENTRIES); memset(c.stage, 0xA5, 4 * STAGE_WORDS); memset(c.mark, 0xA5, T); memset(c.s, 0xA5, 16);
        memset(c.keys, 0xA5, 4 * T); memset(c.cand, 0xA5, 4 * T); memset(c.tokoff, 0xA5, 4 * T);
        memset(c.mlen, 0xA5, 2 * T); memset(c.mdist, 0xA5, 2 * T); memset(c.nxt_a, 0xA5, 2 * T); memset(c.nxt_b, 0xA5, 2 * T);
    }
    ~HostLds()
    {
        free(c.in); free(c.table); free(c.keys); free(c.cand); free(c.tokoff); free(c.stage); free(c.s);
        free(c.mlen); free(c.mdist); free(c.nxt_a); free(c.nxt_b); free(c.mark);
    }
};

int main(int argc, char** argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: deflate_host CASES OUT [ORDERS]\n"); return 2; }
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
        std::vector<uint32_t> lens(n), stored(n);
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
                encode_block(g, lds.c, src, len, member, &lens[b], &stored[b]);
            }
            if (lens[b] < HEADER + FOOTER || lens[b] > len + HEADER + STORED_EXTRA + FOOTER) { printf("FAILED block %u order %d: member of %u bytes\n", b, o, lens[b]); return 1; }
            const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, len);
            for (int k = 0; k < 4; ++k) member[lens[b] - 8 + k] = (uint8_t)(crc >> (8 * k));
            all.insert(all.end(), member, member + lens[b]);
            free(member); free(src);
        }
        const std::string path = std::string(argv[2]) + "." + std::to_string(o);
        FILE* out = fopen(path.c_str(), "wb");
        if (!out) { perror(path.c_str()); return 2; }
        fwrite(&n, 4, 1, out);
        if (n) { fwrite(lens.data(), 4, n, out); fwrite(stored.data(), 4, n, out); fwrite(all.data(), 1, all.size(), out); }
        fclose(out);
    }
    printf("deflate_host: ok, %u blocks, %d orders\n", n, orders);
    return 0;
}
