#!/usr/bin/env python3
"""Distinct images per CNN launch of the bench job (wg, --steps windows): the job's windows are simulated as bench.py simulates
them, their segment-pair records collected, cut into the pipeline's launches -- whole launches of 256 while a window has that
many records, its tail padded to the batch of 64 and split 256 / 128 / 64 as DeviceStage.run splits it -- and every launch goes
through kernels.image_dedup; the live counts are read back.  (In a run the tail of one window can share a launch with the head of
the next, depending on timing: the whole launches, most of the images, do not change.)  Outside any timed run."""
import os, sys
import multiprocessing as mp
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from bench import options_ns, windows_of, wg_job, _simulate_contig

STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
B, SIZES = 64, (256, 128, 64)


def main():
    contigs, _strong = wg_job(STEPS, 1)
    jobs = [dict(name=n, length=l, coverage=30.0, seed=100 + i, kind=None) for i, (n, l) in enumerate(contigs)]
    pool = mp.get_context("fork").Pool(min(len(jobs), 16))           # before the first HIP call
    try:
        made = pool.map(_simulate_contig, jobs, chunksize=1)
    finally:
        pool.close()
        pool.join()
    import torch
    from svision_amd import kernels
    from svision_amd.io import bam
    from svision_amd.sample import Sample
    from svision_amd.collection.output_clusters import collect_pair_lines
    from svision_amd.collection.run_collection import detect_window
    from svision_amd.network.create_batch import PAD_DATA, parse_data_fields
    dev = torch.device("cuda:0")
    pad = np.asarray(parse_data_fields(PAD_DATA.split("_")), np.int32)
    opts = options_ns(B)
    launches = []                                                     # (size, records in it, live)
    for job, (table, genome, _seg) in zip(jobs, made):
        sample = Sample.from_table(table, bam.Fasta(sequences={job["name"]: genome}), 50, device=dev)
        for chrom, lo, hi in windows_of(job["name"], job["length"]):
            _s, clusters = detect_window(opts, sample, chrom, lo, hi)
            lines = collect_pair_lines(clusters, opts)
            rec = np.asarray([ln.record() for ln in lines], np.int32).reshape(-1, 12)
            n = rec.shape[0]
            padded = np.concatenate([rec, np.repeat(pad[None], (-n) % B, axis=0)])
            at = 0
            while at < padded.shape[0]:
                size = next(s for s in SIZES if s <= padded.shape[0] - at)
                d = torch.from_numpy(np.ascontiguousarray(padded[at:at + size])).to(dev)
                live = int(kernels.image_dedup(d)[2].item())
                launches.append((size, min(size, max(0, n - at)), live))
                at += size
            print("window %s:%d-%d  %d records" % (chrom, lo, hi, n), flush=True)
    print("launches %d, records %d" % (len(launches), sum(r for _s, r, _l in launches)))
    for size in SIZES:
        lv = np.asarray([l for s, _r, l in launches if s == size])
        if lv.size:
            q = np.percentile(lv, [0, 10, 25, 50, 75, 90, 100]).astype(int).tolist()
            print("size %3d: %4d launches  live min/p10/p25/median/p75/p90/max %s  mean %.1f  <=32: %d  <=64: %d  <=128: %d"
                  % (size, lv.size, q, lv.mean(), int((lv <= 32).sum()), int((lv <= 64).sum()), int((lv <= 128).sum())))
    big = np.asarray([l for s, _r, l in launches if s > 64])
    print("launches of more than 64 rows: %d, live <= 32 in %d, <= 64 in %d" % (big.size, int((big <= 32).sum()), int((big <= 64).sum())))


if __name__ == "__main__":
    main()
