// svx_stage.hip -- the staging reader of the device-side ingestion behind the C ABI: svx_stage_core.hpp (host C++: the pread
// pool, the slots with head-room, the BGZF block index) with its two callbacks bound to HIP.  upload = hipMemcpyAsync out of the
// pinned slot to the block's place in the group's device buffer, on the caller's "copy" stream, and the slot's own event
// recorded behind it; wait_free = hipEventSynchronize on that event.  No kernel: the bytes cross the bus as the file has them.
//
// Every HIP call is made by the thread that calls svx_stage_open / svx_stage_group / svx_stage_close; the pool's threads only
// pread.  One call stages a whole group, so a caller that holds an interpreter lock gives it up once per group.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/svx.h"
#include "svx_stage_core.hpp"

namespace svx_host { void set_bam_error(const std::string& why); }       // svx_bam.cpp: what svx_bam_error returns on this thread

namespace {

struct Stage {
    svx_stage::StageReader reader;
    svx_stage::Group group;                                  // the tables of the last svx_stage_group, for svx_stage_tables
    std::vector<hipEvent_t> copied;                          // per slot: behind its last upload
    int device = 0;
    hipStream_t stream = nullptr;
};

struct DeviceGuard {                                         // the calling thread's current device, for the length of a call
    int before = -1, want;
    bool ok = true;
    explicit DeviceGuard(int d) : want(d)
    {
        ok = hipGetDevice(&before) == hipSuccess && (before == want || hipSetDevice(want) == hipSuccess);
    }
    ~DeviceGuard() { if (ok && before != want) (void)hipSetDevice(before); }
};

}  // namespace

extern "C" {

void* svx_stage_open(const char* path, int threads, const uint64_t* ranges, int n_ranges, const uint64_t* slot_ptrs, int n_slots,
                     uint64_t slot_bytes, int device, void* copy_stream)
{
    if (!path || !ranges || !slot_ptrs || n_ranges < 0 || n_slots < 2) { svx_host::set_bam_error("svx_stage_open: bad argument"); return nullptr; }
    std::unique_ptr<Stage> s(new Stage());
    s->device = device;
    s->stream = static_cast<hipStream_t>(copy_stream);
    DeviceGuard dev(device);
    if (!dev.ok) { svx_host::set_bam_error("svx_stage_open: no such device"); return nullptr; }
    std::vector<svx_stage::Range> rs;
    for (int i = 0; i < n_ranges; ++i) rs.push_back({ranges[2 * i], ranges[2 * i + 1]});
    std::vector<uint8_t*> slots;
    for (int i = 0; i < n_slots; ++i) slots.push_back(reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(slot_ptrs[i])));
    for (int i = 0; i < n_slots; ++i) {
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            for (hipEvent_t e : s->copied) (void)hipEventDestroy(e);
            svx_host::set_bam_error("svx_stage_open: hipEventCreate failed");
            return nullptr;
        }
        s->copied.push_back(ev);
    }
    if (s->reader.open(path, threads, rs, slots, slot_bytes) != svx_stage::OK) {
        for (hipEvent_t e : s->copied) (void)hipEventDestroy(e);
        svx_host::set_bam_error(s->reader.error());
        return nullptr;
    }
    return s.release();
}

int64_t svx_stage_group(void* stage, uint8_t* d_comp, uint64_t d_comp_bytes, uint64_t* used, double* waits, double* stamps, uint64_t stamps_cap)
{
    Stage* s = static_cast<Stage*>(stage);
    if (!s || !d_comp || !used || !waits) { svx_host::set_bam_error("svx_stage_group: bad argument"); return svx_stage::E_ARG; }
    DeviceGuard dev(s->device);
    if (!dev.ok) { svx_host::set_bam_error("svx_stage_group: no such device"); return svx_stage::E_ARG; }
    const auto upload = [&](int slot, const uint8_t* src, uint64_t dst_off, uint64_t n) -> int {
        if (dst_off > d_comp_bytes || n > d_comp_bytes - dst_off) return -1;                  // (the range is larger than the buffer the caller gave)
        if (hipMemcpyAsync(d_comp + dst_off, src, n, hipMemcpyHostToDevice, s->stream) != hipSuccess) return -1;
        return hipEventRecord(s->copied[slot], s->stream) == hipSuccess ? 0 : -1;
    };
    const auto wait_free = [&](int slot) -> int { return hipEventSynchronize(s->copied[slot]) == hipSuccess ? 0 : -1; };
    const int rc = s->reader.group(upload, wait_free, s->group);
    if (rc != svx_stage::OK) { svx_host::set_bam_error(s->reader.error()); return rc; }
    const svx_stage::Group& g = s->group;
    *used = g.used;
    waits[0] = g.wait_bytes_s; waits[1] = g.wait_free_s; waits[2] = g.total_s;
    if (stamps)
        for (uint64_t i = 0; i < g.ready.size() && i < stamps_cap; ++i) { stamps[2 * i] = g.ready[i]; stamps[2 * i + 1] = g.enqueued[i]; }
    return (int64_t)g.src_off.size();
}

int svx_stage_tables(void* stage, uint64_t* src_off, uint32_t* src_len, uint32_t* isize, uint64_t* coff, uint64_t cap)
{
    const Stage* s = static_cast<const Stage*>(stage);
    if (!s || !src_off || !src_len || !isize || !coff) return SVX_EINVAL;
    const svx_stage::Group& g = s->group;
    const size_t n = g.src_off.size();
    if (cap < n) return SVX_ECAPACITY;
    if (n) {
        memcpy(src_off, g.src_off.data(), 8 * n); memcpy(coff, g.coff.data(), 8 * n);
        memcpy(src_len, g.src_len.data(), 4 * n); memcpy(isize, g.isize.data(), 4 * n);
    }
    return SVX_OK;
}

void svx_stage_close(void* stage)
{
    Stage* s = static_cast<Stage*>(stage);
    if (!s) return;
    s->reader.close();                                       // every worker joined: nothing writes into the slots any more
    DeviceGuard dev(s->device);
    for (hipEvent_t e : s->copied) (void)hipEventDestroy(e);  // (an event whose copy is still on its way is released once it is through)
    delete s;
}

}  // extern "C"
