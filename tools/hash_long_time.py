#!/usr/bin/env python3
"""Per-job time of svx_hash_seeds_long (pieces of more than 2,048 bases) beside the Python aligner's, for profiles/hash_long.txt.

    python tools/hash_long_time.py [--no-host]

Random bases, k = 10, window = 50, the four shapes of the table below; the kernel alone in a launch (1 job) and 32 equal jobs in
one launch, device events around the launch, one warm-up and the median of 5; the Python aligner (tests.hashcases.raw_hit_lists)
once per shape on the same job."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svision_amd import _lib, kernels  # noqa: E402
from tests import hashcases as hc  # noqa: E402

SHAPES = [(2049, 3000), (6000, 9000), (12000, 20000), (65536, 70000)]
K, W = 10, 50


def launch_ms(lib, x, y, n_jobs, dev):
    """Median milliseconds of one svx_hash_seeds_long launch over ``n_jobs`` copies of the job (x, y)."""
    slots = 1
    while slots < 8 * len(y):
        slots *= 2
    cap = 4 * len(y) + 64
    ws = lib.svx_hash_seeds_long_ws_bytes(len(x), len(y))
    desc = np.zeros(n_jobs, kernels.HASH_JOB_DTYPE)
    for j in range(n_jobs):
        desc[j] = (0, len(x), len(x), len(y), j * slots, slots, cap, 2 * cap * j)
    d_bases = torch.from_numpy(np.concatenate([x, y, np.zeros(16, np.uint8)])).to(dev)
    d_jobs = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_table = torch.empty(2 * slots * n_jobs, dtype=torch.int64, device=dev)
    d_hits = torch.empty(2 * cap * 4 * n_jobs, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(2 * n_jobs, dtype=torch.int32, device=dev)
    d_ws = torch.empty(ws * n_jobs, dtype=torch.uint8, device=dev)
    d_ws_off = torch.from_numpy(np.arange(n_jobs, dtype=np.int64) * ws).to(dev)
    sp = kernels._stream_ptr(torch.device(dev))
    times = []
    for _ in range(6):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rc = lib.svx_hash_seeds_long(d_bases.data_ptr(), d_jobs.data_ptr(), n_jobs, d_table.data_ptr(), d_hits.data_ptr(), d_counts.data_ptr(),
                                     d_ws.data_ptr(), d_ws_off.data_ptr(), K, W, kernels.HASH_LONG_MAX_X, sp)
        t1.record()
        _lib.check(rc, "svx_hash_seeds_long")
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return statistics.median(times[1:]), d_counts[:2].tolist()


def main():
    dev = "cuda:0"
    lib = _lib.load()
    print("piece  window  | kernel ms/job, 1 job | kernel ms/job, 32 jobs in a launch | Python aligner ms/job | hits A, B")
    for n, (xl, yl) in enumerate(SHAPES):
        rng = hc._rng("hash_long_time/%d" % n)
        ref, seq = hc.rs(rng, yl), hc.rs(rng, xl)
        x, y = kernels.pack_bases(seq), kernels.pack_bases(ref)
        one, counts = launch_ms(lib, x, y, 1, dev)
        many, _c = launch_ms(lib, x, y, 32, dev)
        host = float("nan")
        if "--no-host" not in sys.argv:
            t = time.perf_counter()
            a, b = hc.raw_hit_lists(ref, seq, K, W)
            host = (time.perf_counter() - t) * 1e3
            assert counts == [len(a), len(b)], (counts, len(a), len(b))
        print("%6d %7d | %8.3f | %8.3f | %8.1f | %s" % (xl, yl, one, many / 32, host, counts), flush=True)


if __name__ == "__main__":
    main()
