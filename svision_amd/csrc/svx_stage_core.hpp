// The staging reader of the device-side ingestion, host C++ only (no HIP): the file ranges of a run's groups go through a ring
// of caller-owned slots -- positional reads by a pool of threads that lives as long as the reader, the BGZF block index of every
// slot on the calling thread -- and leave each slot through an `upload` callback (svx_stage.hip: hipMemcpyAsync; the host test
// program tools/hostwave/stage_main.cpp: memcpy).  Included by svx_bam.cpp too: svx_bgzf_index is bgzf_scan.
//
// A slot is HEAD bytes of head-room followed by P = slot_bytes - HEAD of payload.  Use i of a range [c0, c1) receives the file
// bytes [c0 + i P, c0 + (i + 1) P) at offset HEAD: where a read goes depends on nothing the index finds, so the reads run ahead
// of the index -- into the next range too -- as far as there are free slots, and no byte is read twice.  The head of a block cut
// by the end of use i (shorter than HEAD: a BGZF block is at most 65,536 bytes) goes through a buffer of the reader's own to sit
// just in front of HEAD in use i + 1; a range starts with nothing carried, its c0 is a block boundary.
//
// Threads: the workers only pread and count a use's pieces down.  Everything they share with the calling thread -- the cursor of
// the next piece, the counts, `released`, the flags -- is guarded by one mutex (a piece is 4 MB: a few hundred acquisitions per
// GB).  Every wait is a timed wait that looks at the stop flag again; close() works from any state.
#pragma once

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace svx_stage {

constexpr uint64_t HEAD = 65536;                 // head-room of a slot = the longest BGZF block
constexpr uint64_t PIECE = 4ull << 20;           // a worker's read: up to the next multiple of this many bytes of the FILE
constexpr int MAX_THREADS = 32;

enum : int {
    OK = 0,
    E_ARG = -1,          // a parameter (a slot smaller than two blocks, an empty range, a table that is too small)
    E_READ = -2,         // pread failed, or the range runs past the end of the file
    E_START = -3,        // no BGZF block at the start of a range
    E_MIDDLE = -4,       // not BGZF further inside
    E_UPLOAD = -5,       // a callback failed
    E_STOPPED = -6,      // close() came in between
    E_DONE = -7,         // no range is left
};

inline uint32_t ld16(const uint8_t* p) { uint16_t v; memcpy(&v, p, 2); return v; }
inline uint32_t ld32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

// Whole BGZF blocks at the start of b[0, n), at most cap: emit(k, p, data, end, isize) for block k at b + p, whose payload is
// b[data, end - 8) and which inflates to isize bytes.  -> their number, or -1 (not BGZF at b + *used); *used = the bytes they
// cover (a block cut by the end of the buffer is not counted).
template <class Emit>
inline int64_t bgzf_scan(const uint8_t* b, uint64_t n, uint64_t cap, uint64_t* used, Emit emit)
{
    uint64_t p = 0, k = 0;
    while (p + 18 <= n && k < cap) {
        *used = p;
        if (!(b[p] == 0x1f && b[p + 1] == 0x8b && b[p + 2] == 8 && (b[p + 3] & 4))) return -1;
        const uint32_t xlen = ld16(&b[p + 10]);
        if (p + 12 + xlen > n) break;
        uint32_t bsize = 0;
        bool found = false;
        for (uint64_t q = p + 12; q + 4 <= p + 12 + xlen;) {
            const uint32_t slen = ld16(&b[q + 2]);
            if (b[q] == 'B' && b[q + 1] == 'C' && q + 6 <= p + 12 + xlen) { bsize = ld16(&b[q + 4]); found = true; }
            q += 4 + slen;
        }
        if (!found) return -1;
        if (p + bsize + 1 > n) break;
        const uint64_t data = p + 12 + xlen, end = p + bsize + 1;
        if (end < data + 8) return -1;
        emit(k, p, data, end, ld32(&b[end - 4]));
        ++k;
        p = end;
    }
    *used = p;
    return (int64_t)k;
}

struct Range { uint64_t c0, c1; };

struct Group {                                   // what one group() call found: the tables of the range's whole blocks
    std::vector<uint64_t> src_off, coff;         // payload offset from the range's c0 (= its place in the device buffer); file offset
    std::vector<uint32_t> src_len, isize;
    uint64_t used = 0;                           // bytes those blocks cover, from c0
    double wait_bytes_s = 0, wait_free_s = 0, total_s = 0;
    std::vector<double> ready, enqueued;         // per slot use: seconds since open() at which its bytes were there / its upload was issued
    void clear() { src_off.clear(); coff.clear(); src_len.clear(); isize.clear(); ready.clear(); enqueued.clear(); used = 0; wait_bytes_s = wait_free_s = total_s = 0; }
};

class StageReader {
public:
    using Upload = std::function<int(int slot, const uint8_t* src, uint64_t dst_off, uint64_t n)>;     // -> 0, or the group fails
    using WaitFree = std::function<int(int slot)>;                                                      // the slot's last upload has left it

    StageReader() = default;
    StageReader(const StageReader&) = delete;
    StageReader& operator=(const StageReader&) = delete;
    ~StageReader() { close(); }

    // -> OK or E_ARG / E_READ with error() set; the pool starts reading at once
    int open(const char* path, int threads, const std::vector<Range>& ranges, const std::vector<uint8_t*>& slots, uint64_t slot_bytes)
    {
        if (fd_ >= 0 || !workers_.empty()) return fail(E_ARG, "the reader is open");
        if (slots.size() < 2 || slot_bytes < 2 * HEAD) return fail(E_ARG, "a staging ring is at least two slots of 128 KB");
        for (const Range& r : ranges)
            if (r.c1 <= r.c0) return fail(E_ARG, "empty file range");
        fd_ = ::open(path, O_RDONLY);
        if (fd_ < 0) return fail(E_READ, std::string("cannot open ") + path);
        ranges_ = ranges; slots_ = slots; payload_ = slot_bytes - HEAD;
        first_use_.assign(1, 0);
        for (const Range& r : ranges_) first_use_.push_back(first_use_.back() + (r.c1 - r.c0 + payload_ - 1) / payload_);
        uses_.assign(first_use_.back(), Use());
        for (size_t r = 0; r < ranges_.size(); ++r)
            for (uint64_t u = first_use_[r]; u < first_use_[r + 1]; ++u) {
                Use& x = uses_[u];
                x.off = ranges_[r].c0 + (u - first_use_[r]) * payload_;
                x.len = std::min(payload_, ranges_[r].c1 - x.off);
                x.pieces_left = (int)((x.off + x.len + PIECE - 1) / PIECE - x.off / PIECE);
            }
        // the uses [released_, released_ + slots) may be read into: half the ring ahead of the use the caller is at, the other
        // half for the uploads that are still on their way (measured with 64 MB slots: the ring is drained at the bus's rate --
        // the calling thread waits for copies, never for bytes -- and 12 or 16 slots instead of 8 did not shorten a run)
        ahead_ = std::max<uint64_t>(1, slots_.size() / 2);
        carry_buf_.assign(HEAD, 0);
        carry_ = 0; next_range_ = 0; released_ = released_local_ = 0; cur_use_w_ = 0; cur_at_ = 0; stop_ = false; failed_ = OK;
        t0_ = std::chrono::steady_clock::now();
        threads = std::max(1, std::min(threads, MAX_THREADS));
        for (int t = 0; t < threads; ++t) workers_.emplace_back([this] { work(); });
        return OK;
    }

    // The calling thread: the next range, slot by slot -- wait for the bytes, carry, index, upload -- into `g`.  -> OK or a code
    // with error() set; after a failure every further call fails the same way and close() still works.
    int group(const Upload& upload, const WaitFree& wait_free, Group& g)
    {
        g.clear();
        if (failed_ != OK) return failed_;
        if (next_range_ >= ranges_.size()) return fail(E_DONE, "no file range is left");
        const auto t_in = std::chrono::steady_clock::now();
        const size_t r = next_range_++;
        const Range range = ranges_[r];
        carry_ = 0;
        for (uint64_t u = first_use_[r]; u < first_use_[r + 1]; ++u) {
            // uses up to u + ahead_ may be read: the uploads of the uses that held their slots before have to be through
            const uint64_t want_released = u + ahead_ + 1 > slots_.size() ? u + ahead_ + 1 - slots_.size() : 0;
            while (released_local_ < std::min<uint64_t>(want_released, u)) {
                const auto t_w = std::chrono::steady_clock::now();
                if (wait_free((int)(released_local_ % slots_.size())) != 0) return fail(E_UPLOAD, "waiting for a staging slot's copy failed");
                g.wait_free_s += since(t_w);
                ++released_local_;
                std::lock_guard<std::mutex> lk(m_);
                released_ = released_local_;
                cv_work_.notify_all();
            }
            const auto t_b = std::chrono::steady_clock::now();
            int err = OK;
            {
                std::unique_lock<std::mutex> lk(m_);
                while (uses_[u].pieces_left > 0 && uses_[u].err == OK && !stop_) nap(cv_ready_, lk);
                err = stop_ ? (int)E_STOPPED : uses_[u].err;
            }
            g.wait_bytes_s += since(t_b);
            if (err == E_STOPPED) return fail(E_STOPPED, "the staging reader was closed");
            if (err != OK) return fail(E_READ, "short read at file offset " + std::to_string(uses_[u].off));
            g.ready.push_back(since(t0_));
            const Use& x = uses_[u];
            uint8_t* slot = slots_[u % slots_.size()];
            if (carry_) memcpy(slot + HEAD - carry_, carry_buf_.data(), carry_);
            const uint8_t* at = slot + HEAD - carry_;
            const uint64_t n = carry_ + x.len, base = x.off - carry_ - range.c0;      // `at` lies at `base` of the device buffer
            uint64_t used = 0;
            const int64_t k = bgzf_scan(at, n, ~0ull, &used, [&](uint64_t, uint64_t p, uint64_t data, uint64_t end, uint32_t isz) {
                g.src_off.push_back(base + data);
                g.src_len.push_back((uint32_t)(end - 8 - data));
                g.isize.push_back(isz);
                g.coff.push_back(range.c0 + base + p);
            });
            const bool last = u + 1 == first_use_[r + 1];
            if (k < 0 || (!last && n - used > HEAD))                  // (more than a block's length without a block: not BGZF either)
                return fail(u == first_use_[r] && used == 0 ? E_START : E_MIDDLE, "no BGZF block at file offset " + std::to_string(range.c0 + base + used));
            if (used) {
                if (upload((int)(u % slots_.size()), at, base, used) != 0) return fail(E_UPLOAD, "the upload of a staging slot failed");
                g.used = base + used;
            }
            g.enqueued.push_back(since(t0_));
            carry_ = last ? 0 : n - used;
            if (carry_) memcpy(carry_buf_.data(), at + used, carry_);
        }
        if (g.src_off.empty()) return fail(E_START, "no BGZF block at file offset " + std::to_string(range.c0));
        g.total_s = since(t_in);
        return OK;
    }

    // From any state -- in the middle of a range, after an error, with reads outstanding --: the workers are told to stop and
    // joined (one that is inside a pread finishes it: the slots have to outlive this call), the file is closed.
    void close()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_work_.notify_all();
        cv_ready_.notify_all();
        for (auto& th : workers_) th.join();
        workers_.clear();
        if (fd_ >= 0) ::close(fd_);
        fd_ = -1;
    }

    // Another thread may ask a group() that is waiting to give up (it returns E_STOPPED); close() is still the caller's to make.
    void request_stop()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_work_.notify_all();
        cv_ready_.notify_all();
    }

    const std::string& error() const { return error_; }
    size_t n_workers() const { return workers_.size(); }

private:
    struct Use {                                 // one filling of a slot: file bytes [off, off + len) to slot + HEAD
        uint64_t off = 0, len = 0;
        int pieces_left = 0, err = OK;
    };

    static double since(std::chrono::steady_clock::time_point t)
    {
        return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
    }

    // A wait with a way out: at most 50 ms, then the caller looks at its condition and the stop flag again.  (Against the system
    // clock: that is pthread_cond_timedwait, which ThreadSanitizer follows; the steady clock's pthread_cond_clockwait it does not
    // know everywhere, and reports the mutex as locked twice.  A clock that is set only makes one nap shorter or longer.)
    static void nap(std::condition_variable& cv, std::unique_lock<std::mutex>& lk)
    {
        cv.wait_until(lk, std::chrono::system_clock::now() + std::chrono::milliseconds(50));
    }

    int fail(int code, const std::string& why)
    {
        error_ = why;
        if (code != E_ARG && code != E_DONE) failed_ = code;
        return code;
    }

    void work()
    {
        std::unique_lock<std::mutex> lk(m_);
        while (!stop_) {
            if (cur_use_w_ >= uses_.size() || cur_use_w_ >= released_ + slots_.size()) {
                nap(cv_work_, lk);
                continue;
            }
            const uint64_t u = cur_use_w_;
            Use& x = uses_[u];
            const uint64_t lo = x.off + cur_at_, hi = std::min(x.off + x.len, (lo / PIECE + 1) * PIECE);
            cur_at_ += hi - lo;
            if (cur_at_ == x.len) { ++cur_use_w_; cur_at_ = 0; }
            uint8_t* dst = slots_[u % slots_.size()] + HEAD + (lo - x.off);
            lk.unlock();
            bool ok = true;
            for (uint64_t done = lo; done < hi;) {
                const ssize_t got = pread(fd_, dst + (done - lo), hi - done, (off_t)done);
                if (got <= 0) { ok = false; break; }
                done += (uint64_t)got;
            }
            lk.lock();
            if (!ok) x.err = E_READ;
            if (--x.pieces_left == 0 || !ok) cv_ready_.notify_all();
        }
    }

    int fd_ = -1;
    std::vector<Range> ranges_;
    std::vector<uint8_t*> slots_;
    uint64_t payload_ = 0, ahead_ = 1;
    std::vector<uint64_t> first_use_;            // [n_ranges + 1]: the uses of range r are [first_use_[r], first_use_[r + 1])
    std::vector<Use> uses_;                      // .pieces_left / .err: under m_
    std::vector<uint8_t> carry_buf_;
    uint64_t carry_ = 0;
    size_t next_range_ = 0;
    uint64_t released_local_ = 0;                // the calling thread's copy of released_
    int failed_ = OK;
    std::string error_;
    std::chrono::steady_clock::time_point t0_;

    std::mutex m_;
    std::condition_variable cv_work_, cv_ready_;
    uint64_t released_ = 0;                      // under m_: the workers may fill the uses below released_ + slots
    uint64_t cur_use_w_ = 0, cur_at_ = 0;        // under m_: the next piece starts at byte cur_at_ of use cur_use_w_
    bool stop_ = false;                          // under m_
    std::vector<std::thread> workers_;
};

}  // namespace svx_stage
