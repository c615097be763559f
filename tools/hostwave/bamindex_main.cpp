// svx_bam_find_starts and svx_bam_walk_offsets (svision_amd/csrc/svx_bamindex.hip) as a host program: the kernel file itself, compiled
// against tools/hostwave/hip/hip_runtime.h, run on case files (tests/test_bamindex_host_cpu.py writes them) whose inflated bytes
// lie in a heap block of exactly their size.  Build: g++ -std=c++20 -O1 -fsanitize=address,undefined -x c++ -I tools/hostwave -pthread.
#include "../../svision_amd/csrc/svx_bamindex.hip"
#include <cstdio>
#include <cstdlib>
// case file: u64 n_blocks, entry, n_ref, total; dst_off[n+1] u64; ref_len[n_ref] i32 (padded to 8); raw[total] (padded to 8); first[n] u64; exit[2] u64
int main(int argc, char** argv)
{
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { perror(argv[a]); return 2; }
        uint64_t h[4];
        if (fread(h, 8, 4, f) != 4) return 2;
        const uint64_t n = h[0], entry = h[1], n_ref = h[2], total = h[3];
        std::vector<uint64_t> dst(n + 1), want(n), want_exit(2), got(n, 7), got_exit(2, 7);
        std::vector<int32_t> ref_len((n_ref + 1) / 2 * 2 + 2);
        fread(dst.data(), 8, n + 1, f);
        fread(ref_len.data(), 4, (n_ref + 1) / 2 * 2, f);
        // exactly `total` bytes on the heap: the sanitizer sees every read behind the range's end
        uint8_t* raw = (uint8_t*)malloc(total ? total : 1);
        fread(raw, 1, total, f);
        fseek(f, (long)((8 - total % 8) % 8), SEEK_CUR);
        fread(want.data(), 8, n, f);
        fread(want_exit.data(), 8, 2, f);
        fclose(f);
        const size_t ws_bytes = svx_bam_find_starts_ws_bytes((uint32_t)n);
        void* ws = aligned_alloc(16, (ws_bytes + 15) / 16 * 16);
        memset(ws, 0xA5, ws_bytes);
        const int rc = svx_bam_find_starts(raw, dst.data(), (uint32_t)n, entry, (uint32_t)n_ref, ref_len.data(), got.data(), got_exit.data(), ws, ws_bytes, nullptr);
        uint64_t diff = 0;
        for (uint64_t b = 0; b < n; ++b) diff += got[b] != want[b];
        const bool ok = rc == 0 && got_exit[0] == want_exit[0] && got_exit[1] == want_exit[1] && (want_exit[1] != 0 || diff == 0);
        printf("%s: %s  rc %d, %llu blocks, %llu differ, exit %llu/%llu want %llu/%llu\n", argv[a], ok ? "ok" : "FAILED", rc, (unsigned long long)n,
               (unsigned long long)diff, (unsigned long long)got_exit[0], (unsigned long long)got_exit[1], (unsigned long long)want_exit[0], (unsigned long long)want_exit[1]);
        if (!ok) for (uint64_t b = 0; b < n && bad < 40; ++b) if (got[b] != want[b]) { printf("  block %llu [%llu, %llu): got %lld want %lld\n", (unsigned long long)b, (unsigned long long)dst[b], (unsigned long long)dst[b + 1], (long long)got[b], (long long)want[b]); ++bad; }
        if (ok && want_exit[1] == 0) {                            // svx_bam_walk_offsets over the compacted starts against a plain walk
            std::vector<uint64_t> starts;
            for (uint64_t b = 0; b < n; ++b) if (got[b] != ~0ull) starts.push_back(got[b]);
            if (starts.empty() || starts.back() != got_exit[0]) starts.push_back(got_exit[0]);
            const uint32_t ns = (uint32_t)starts.size() - 1;
            std::vector<uint64_t> base(3 * (ns + 1)), plain;
            uint64_t k = 0;
            for (uint32_t i = 0; i < ns; ++i) {
                base[3 * i] = k;
                for (uint64_t p = starts[i]; p < starts[i + 1]; p += 4 + (uint64_t)(raw[p] | raw[p + 1] << 8 | raw[p + 2] << 16 | (uint32_t)raw[p + 3] << 24)) { plain.push_back(p); ++k; }
            }
            std::vector<uint64_t> off(k + 1, 7);
            const int rc2 = ns ? svx_bam_walk_offsets(raw, starts.data(), ns, base.data(), off.data(), nullptr) : 0;
            off.resize(k);
            const bool ok2 = rc2 == 0 && off == plain;
            printf("  walk_offsets: %s, %llu records over %u starts\n", ok2 ? "ok" : "FAILED", (unsigned long long)k, ns);
            bad += !ok2;
        }
        bad += !ok;
        free(raw); free(ws);
    }
    return bad ? 1 : 0;
}
