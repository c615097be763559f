// scatter_segments_kernel (svision_amd/csrc/svx_recsort.hip) without a GPU: the lane routine of svx_recsort_core.hpp -- the code the
// kernel runs -- as a loop over the 64 lanes of every input record's wave.  Built with -fsanitize=address,undefined: the source lies
// in a heap block of exactly the size include/svx.h asks for (its bytes, readable up to the next multiple of 4), the destination in
// one of exactly the window's bytes, both at the alignment under test; every read or write outside is reported.
// Build: g++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all.
//
// usage: scatter_host LENGTH...     the segments' lengths in input order.  Runs every source skew x destination alignment with all
//                                   ranks in the window, one window in the middle, and one wrong length.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../svision_amd/csrc/svx_recsort_core.hpp"

static int g_failed = 0;

struct Case { uint32_t skew, align, rank_lo, rank_hi; int64_t wrong; };     // wrong: the rank whose output length is off by one, or -1

static void run(const std::vector<int64_t>& len, const std::vector<uint32_t>& order, const Case& c)
{
    const size_t n = len.size();
    std::vector<uint32_t> rank(n);
    for (size_t r = 0; r < n; ++r) rank[order[r]] = (uint32_t)r;
    // the source: `skew` bytes in front of the first segment, so that source offsets take every value mod 4
    std::vector<int64_t> src_off(n + 1), off_out(n + 1);
    src_off[0] = c.skew;
    for (size_t i = 0; i < n; ++i) src_off[i + 1] = src_off[i] + len[i];
    off_out[0] = 0;
    for (size_t r = 0; r < n; ++r) off_out[r + 1] = off_out[r] + len[order[r]];
    const int64_t src_bytes = (src_off[n] + 3) / 4 * 4;
    uint8_t* src = static_cast<uint8_t*>(aligned_alloc(4, (size_t)(src_bytes ? src_bytes : 4)));
    for (int64_t p = 0; p < src_bytes; ++p) src[p] = (uint8_t)(p * 131 + (p >> 8) * 7 + 1);
    // the output's offsets as the kernel is given them: rank `wrong` a byte longer than its record, every later rank a byte on
    std::vector<int64_t> off_used = off_out;
    if (c.wrong >= 0) for (size_t r = (size_t)c.wrong + 1; r <= n; ++r) off_used[r] += 1;
    // the destination: a heap block of exactly the window's bytes behind c.align sentinel bytes, so that the window's first byte
    // lies at address = c.align (mod 4)
    const int64_t out_base = off_used[c.rank_lo], w_bytes = off_used[c.rank_hi] - out_base;
    uint8_t* exact = static_cast<uint8_t*>(malloc((size_t)(w_bytes + c.align ? w_bytes + c.align : 1)));
    uint8_t* dst = exact + c.align;
    memset(exact, 0xA5, (size_t)(w_bytes + c.align));
    int32_t status = 0;
    for (uint64_t i = 0; i < n; ++i)
        for (uint32_t lane = 0; lane < svx_recsort::WAVE; ++lane)
            svx_recsort::scatter_record(src, src_off.data(), rank.data(), c.rank_lo, c.rank_hi, off_used.data(), out_base, dst, i, lane, &status);
    // expected: every record of the window at its place; the place of the wrong one and the sentinels in front still 0xA5
    std::vector<uint8_t> want((size_t)(w_bytes + c.align) + 1, 0xA5);
    for (uint32_t r = c.rank_lo; r < c.rank_hi; ++r)
        if ((int64_t)r != c.wrong) memcpy(want.data() + c.align + (off_used[r] - out_base), src + src_off[order[r]], (size_t)len[order[r]]);
    const bool bytes_ok = memcmp(want.data(), exact, (size_t)(w_bytes + c.align)) == 0;
    const bool ok = bytes_ok && status == (c.wrong >= 0 ? 1 : 0);
    printf("skew %u align %u window [%u, %u) wrong %lld: %s  status %d, %lld bytes\n", c.skew, c.align, c.rank_lo, c.rank_hi, (long long)c.wrong,
           ok ? "ok" : "FAILED", status, (long long)w_bytes);
    g_failed += !ok;
    free(exact);
    free(src);
}

int main(int argc, char** argv)
{
    std::vector<int64_t> len;
    for (int a = 1; a < argc; ++a) len.push_back(atoll(argv[a]));
    const uint32_t n = (uint32_t)len.size();
    if (n < 8) { fprintf(stderr, "usage: scatter_host LENGTH... (at least 8)\n"); return 2; }
    // a fixed permutation: a multiplicative step that is coprime to n
    std::vector<uint32_t> order(n);
    uint32_t step = 7;
    auto gcd = [](uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; };
    while (gcd(step, n) != 1) ++step;
    for (uint32_t r = 0; r < n; ++r) order[r] = (uint32_t)(((uint64_t)r * step + 3) % n);
    for (uint32_t skew = 0; skew < 4; ++skew)
        for (uint32_t align = 0; align < 4; ++align) {
            run(len, order, Case{skew, align, 0, n, -1});
            run(len, order, Case{skew, align, n / 3, 2 * n / 3, -1});
        }
    // one wrong length: the longest record of the middle window, and the last rank of all
    uint32_t longest = n / 3;
    for (uint32_t r = n / 3; r < 2 * n / 3; ++r) if (len[order[r]] > len[order[longest]]) longest = r;
    run(len, order, Case{1, 3, n / 3, 2 * n / 3, (int64_t)longest});
    run(len, order, Case{2, 1, 0, n, (int64_t)n - 1});
    printf("%d failures\n", g_failed);
    return g_failed ? 1 : 0;
}
