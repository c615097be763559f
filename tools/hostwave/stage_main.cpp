// The staging reader (svision_amd/csrc/svx_stage_core.hpp) without a GPU, for AddressSanitizer / UBSan and ThreadSanitizer builds
// (tests/test_stage_reader_cpu.py).  The "device" is a heap buffer of exactly each range's size, every slot a heap block of
// exactly slot_bytes.  The upload is LATE on purpose, the way a copy on a stream may be: `upload` only notes what is to be copied,
// the memcpy happens when the reader asks for the slot back (wait_free, which sleeps a millisecond now and then) or, for the
// slots it never asked back, before the comparison -- a worker that wrote into a slot too early would be seen in the bytes.
//
//   stage_host PATH OUT THREADS RANGES CONFIGS MODE
//     RANGES   c0-c1,c0-c1,...          file ranges, one group() each
//     CONFIGS  BYTESxSLOTS,...          ring shapes; every one is run over all ranges
//     MODE     run         every range; the bytes of each == the file's, the tables of every config == the first one's, which are
//                          written to OUT.<range> (u64 n, u64 used, u64 src_off[n], u64 coff[n], u32 src_len[n], u32 isize[n])
//              stop3       the reader is asked to stop from inside the third upload, then closed
//              early       closed right after the open, reads outstanding
//              abandon     closed after the first range, the reads of the next one outstanding
//   Prints per config and range "range R: rc CODE blocks N used U [text]" and "closed: workers 0"; exit status 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../svision_amd/csrc/svx_stage_core.hpp"

using svx_stage::Group;
using svx_stage::Range;
using svx_stage::StageReader;

namespace {

std::vector<std::string> split(const std::string& s, char sep)
{
    std::vector<std::string> out;
    size_t at = 0;
    while (at <= s.size()) {
        const size_t e = std::min(s.find(sep, at), s.size());
        if (e > at) out.push_back(s.substr(at, e - at));
        at = e + 1;
    }
    return out;
}

struct Pending { const uint8_t* src = nullptr; uint8_t* dst = nullptr; uint64_t n = 0; };

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 7) { fprintf(stderr, "usage: stage_host PATH OUT THREADS RANGES CONFIGS MODE\n"); return 2; }
    const std::string path = argv[1], out = argv[2], mode = argv[6];
    const int threads = atoi(argv[3]);
    std::vector<Range> ranges;
    for (const auto& r : split(argv[4], ',')) {
        const auto ab = split(r, '-');
        ranges.push_back({strtoull(ab[0].c_str(), nullptr, 10), strtoull(ab[1].c_str(), nullptr, 10)});
    }
    std::vector<uint8_t> file;
    {
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); return 2; }
        fseek(f, 0, SEEK_END);
        file.resize((size_t)ftell(f));
        fseek(f, 0, SEEK_SET);
        if (!file.empty() && fread(file.data(), 1, file.size(), f) != file.size()) return 2;
        fclose(f);
    }
    bool bad = false;
    std::vector<Group> first(ranges.size());
    bool have_first = false;
    for (const auto& cfg : split(argv[5], ',')) {
        const auto sn = split(cfg, 'x');
        const uint64_t slot_bytes = strtoull(sn[0].c_str(), nullptr, 10);
        const int n_slots = atoi(sn[1].c_str());
        printf("config %llu x %d\n", (unsigned long long)slot_bytes, n_slots);
        std::vector<uint8_t*> slots;
        for (int i = 0; i < n_slots; ++i) slots.push_back(static_cast<uint8_t*>(malloc(slot_bytes)));
        std::vector<uint8_t*> dev;
        for (const Range& r : ranges) dev.push_back(static_cast<uint8_t*>(calloc(r.c1 - r.c0, 1)));
        std::vector<Pending> pending(n_slots);
        auto settle = [&](int slot) {
            Pending& p = pending[slot];
            if (p.n) memcpy(p.dst, p.src, p.n);
            p = Pending();
        };
        StageReader reader;
        int rc = reader.open(path.c_str(), threads, ranges, slots, slot_bytes);
        if (rc != svx_stage::OK) {
            printf("open: rc %d %s\n", rc, reader.error().c_str());
        } else if (mode == "early") {
            reader.close();
        } else {
            std::vector<Group> groups(ranges.size());
            size_t done = 0;
            for (size_t r = 0; r < ranges.size(); ++r) {
                int uploads = 0, waits = 0;
                const uint64_t size = ranges[r].c1 - ranges[r].c0;
                auto upload = [&](int slot, const uint8_t* src, uint64_t dst_off, uint64_t n) -> int {
                    if (dst_off > size || n > size - dst_off) { printf("FAILED: upload [%llu, +%llu) outside a range of %llu\n", (unsigned long long)dst_off, (unsigned long long)n, (unsigned long long)size); return -1; }
                    if (src < slots[slot] || src + n > slots[slot] + slot_bytes) { printf("FAILED: upload source outside slot %d\n", slot); return -1; }
                    settle(slot);                              // (a slot handed out twice without wait_free would show here as an early copy: it is not)
                    pending[slot] = Pending{src, dev[r] + dst_off, n};
                    if (mode == "stop3" && ++uploads == 3) reader.request_stop();
                    return 0;
                };
                auto wait_free = [&](int slot) -> int {
                    if (++waits % 4 == 0) std::this_thread::sleep_for(std::chrono::milliseconds(1));
                    settle(slot);
                    return 0;
                };
                rc = reader.group(upload, wait_free, groups[r]);
                printf("range %zu: rc %d blocks %zu used %llu %s\n", r, rc, groups[r].src_off.size(), (unsigned long long)groups[r].used, rc ? reader.error().c_str() : "");
                if (rc != svx_stage::OK) break;
                ++done;
                if (mode == "abandon") break;
            }
            reader.close();
            for (int i = 0; i < n_slots; ++i) settle(i);
            if (mode == "run")
                for (size_t r = 0; r < done; ++r) {
                    const Group& g = groups[r];
                    if (ranges[r].c0 + g.used > file.size() || memcmp(dev[r], file.data() + ranges[r].c0, g.used) != 0) {
                        printf("FAILED: the bytes of range %zu differ from the file's\n", r);
                        bad = true;
                    }
                    if (have_first && (g.src_off != first[r].src_off || g.coff != first[r].coff || g.src_len != first[r].src_len || g.isize != first[r].isize || g.used != first[r].used)) {
                        printf("FAILED: the tables of range %zu differ from the first ring's\n", r);
                        bad = true;
                    }
                }
            if (mode == "run" && !have_first && done == ranges.size()) {
                first = groups;
                have_first = true;
                for (size_t r = 0; r < ranges.size(); ++r) {
                    const Group& g = groups[r];
                    FILE* f = fopen((out + "." + std::to_string(r)).c_str(), "wb");
                    if (!f) return 2;
                    const uint64_t head[2] = {g.src_off.size(), g.used};
                    fwrite(head, 8, 2, f);
                    fwrite(g.src_off.data(), 8, g.src_off.size(), f);
                    fwrite(g.coff.data(), 8, g.coff.size(), f);
                    fwrite(g.src_len.data(), 4, g.src_len.size(), f);
                    fwrite(g.isize.data(), 4, g.isize.size(), f);
                    fclose(f);
                }
            }
        }
        printf("closed: workers %zu\n", reader.n_workers());
        for (uint8_t* p : slots) free(p);
        for (uint8_t* p : dev) free(p);
    }
    return bad ? 1 : 0;
}
