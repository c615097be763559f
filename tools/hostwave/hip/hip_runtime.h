// Host stand-in for <hip/hip_runtime.h>, enough for kernels that use blockIdx / threadIdx, __ballot and __ffsll and no LDS: a launch
// runs every wave as 64 host threads, __ballot is a barrier exchange between them.  It lets a kernel file be compiled as plain C++
// (g++ -std=c++20 -I tools/hostwave -x c++) into a stand-alone program with its own main -- with -fsanitize=address,undefined every
// read a kernel makes behind a buffer's end is reported on a machine without a GPU (tools/hostwave/bamindex_main.cpp,
// tests/test_bamindex_host_cpu.py).  Not a model of the device: no timing, no memory model, one wave at a time.
#pragma once
#include <atomic>
#include <barrier>
#include <cstdint>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
typedef void* hipStream_t;
enum { hipSuccess = 0 };
inline int hipGetLastError() { return 0; }
struct EmuWave { std::barrier<> bar{64}; std::atomic<uint64_t> mask{0}; };
inline thread_local dim3 blockIdx, threadIdx;
inline thread_local EmuWave* emu_wave = nullptr;
inline uint64_t __ballot(bool p)
{
    EmuWave& w = *emu_wave;
    const unsigned lane = threadIdx.x & 63u;
    if (p) w.mask.fetch_or(1ull << lane);
    w.bar.arrive_and_wait();
    const uint64_t r = w.mask.load();
    w.bar.arrive_and_wait();
    if (lane == 0) w.mask.store(0);
    w.bar.arrive_and_wait();
    return r;
}
inline int __ffsll(unsigned long long m) { return __builtin_ffsll((long long)m); }
template <class K, class... A>
void emu_launch(K kernel, dim3 grid, dim3 block, A... args)
{
    for (unsigned bx = 0; bx < grid.x; ++bx)
        for (unsigned w0 = 0; w0 < block.x; w0 += 64) {
            EmuWave wave;
            std::vector<std::thread> lanes;
            for (unsigned l = 0; l < 64; ++l)
                lanes.emplace_back([&, l] {
                    blockIdx = dim3(bx); threadIdx = dim3(w0 + l); emu_wave = &wave;
                    struct Drop { EmuWave& w; ~Drop() { w.bar.arrive_and_drop(); } } drop{wave};
                    kernel(args...);
                });
            for (auto& t : lanes) t.join();
        }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)
