#!/usr/bin/env python
"""Ingestion WITH the read bases (--hash / --graph), device engine against host engine, on a bench-style file.

    python tools/ingest_seq_ab.py build FILE.bam [--windows 20] [--coverage 30]
        a file like bench.py's: a prefix of every GRCh38 chromosome (bench.job_contigs), simulated HiFi reads, written by
        encode_reference_segment(seq="random") -- random bases, QUAL, 64 KB blocks -- + its .bai and FILE.bam.json (the windows)
    python tools/ingest_seq_ab.py run FILE.bam --engine cpu|gpu
        ONE pass in this process: a ChromosomeFeed with with_seq on (options.hash) over the file's windows; timed from opening
        the file to the last spill being complete (host engine: to the last hand-over -- its tables are complete when handed
        over).  The HIP context and libsvx.so are up before the clock starts.  Prints one JSON line.
    python tools/ingest_seq_ab.py ab FILE.bam [--runs 3]
        `run` with the host and the device engine alternately, a fresh process each, and the verdict for "auto": the device
        engine only if its median is below the host engine's FASTEST run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build(args):
    import multiprocessing as mp
    import bench                                            # (imported for job_contigs / _simulate_contig: the file is built the bench's way)
    from svision_amd.io import bam
    contigs = bench.job_contigs(args.windows)
    jobs = [dict(name=n, length=l, coverage=args.coverage, seed=100 + i, kind=None, e2e=(i, l)) for i, (n, l) in enumerate(contigs)]
    pool = mp.get_context("fork").Pool(min(len(jobs), args.procs))
    try:
        made = pool.map(bench._simulate_contig, jobs, chunksize=1)
    finally:
        pool.close()
        pool.join()
    bam.write_bam_segments(args.file, [n for n, _l in contigs], [l for _n, l in contigs], [seg for _t, _g, seg in made])
    windows = [w for n, l in contigs for w in bench.windows_of(n, l)]
    with open(args.file + ".json", "w") as f:
        json.dump({"windows": windows, "records": int(sum(len(t) for t, _g, _s in made)), "inflated": int(sum(s["inflated"] for _t, _g, s in made))}, f)
    print("built %s: %d windows, %.2f GB, %.2f GB inflated" % (args.file, len(windows), os.path.getsize(args.file) / 1e9,
                                                              sum(s["inflated"] for _t, _g, s in made) / 1e9))


def run(args):
    import types
    import numpy as np
    import torch
    from svision_amd import _lib, ingest
    from svision_amd.io import bam
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev).add_(1).cpu()               # the HIP context, a first kernel, a first read-back
    _lib.load()
    with open(args.file + ".json") as f:
        meta = json.load(f)
    tasks = {}
    for c, a, b in meta["windows"]:
        tasks.setdefault(c, []).append((a, b))
    opts = types.SimpleNamespace(hash=True, graph=False, contig=False, min_sv_size=50)
    t0 = time.perf_counter()
    head = bam.read_bam_header(args.file)
    chroms = [c for c in head.references if c in tasks]
    feed = ingest.ChromosomeFeed(args.file, bam.Fasta(sequences={}), opts, chroms, head.references, head.lengths, device=dev,
                                 index=bam.find_index(args.file), threads=ingest.decode_threads(), engine=args.engine, tasks=tasks)
    try:
        seq_bytes, records, t_first = 0, 0, None
        while not feed.finished:
            feed.poll(block=True)
            if t_first is None and feed.samples:
                t_first = time.perf_counter() - t0
        t_handover = time.perf_counter() - t0
        for ents in feed.samples.values():
            for _lo, _hi, _key, smp, m in ents:
                if m is not None and m.get("spilled") is not None:
                    m["spilled"].wait(timeout=300)
        t_all = time.perf_counter() - t0
        if feed.error is not None:
            raise feed.error
        for ents in feed.samples.values():
            for _lo, _hi, _key, smp, _m in ents:
                sp = smp.table.seq_packed
                records += len(smp.table)
                seq_bytes += 0 if sp is None else (sp.size if hasattr(sp, "size") else len(sp))
        # (a spot check that the bases are there: the first and the last record of the first part)
        first = next(iter(feed.samples.values()))[0][3].table
        got = [first.query_sequence(i) for i in (0, len(first) - 1)]
        assert all(s is not None and len(s) == int(first.l_seq[i]) for s, i in zip(got, (0, len(first) - 1)))
        print(json.dumps({"engine": feed.stats["engine"], "seconds": round(t_all, 4), "first_part_s": round(t_first, 4), "last_handover_s": round(t_handover, 4),
                          "parts": int(feed.stats["slices"]), "replans": int(feed.stats["replans"]), "records": records, "seq_bytes": int(seq_bytes),
                          "kind": type(first.seq_packed).__name__}))
    finally:
        feed.close()


def ab(args):
    times = {"cpu": [], "gpu": []}
    for i in range(args.runs):
        for engine in ("cpu", "gpu"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "run", args.file, "--engine", engine], capture_output=True, text=True,
                               timeout=args.timeout)
            if r.returncode != 0:                              # nothing more is started behind a failed run
                sys.stdout.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit("run %d, engine %s: exit status %d" % (i + 1, engine, r.returncode))
            line = json.loads(r.stdout.strip().splitlines()[-1])
            assert line["engine"] == engine, line
            times[engine].append(line["seconds"])
            print("run %d  %s" % (i + 1, json.dumps(line)), flush=True)
    med = {e: sorted(v)[len(v) // 2] for e, v in times.items()}
    print("host   (cpu): %s  median %.4f  fastest %.4f" % (" ".join("%.4f" % v for v in times["cpu"]), med["cpu"], min(times["cpu"])))
    print("device (gpu): %s  median %.4f  fastest %.4f" % (" ".join("%.4f" % v for v in times["gpu"]), med["gpu"], min(times["gpu"])))
    verdict = med["gpu"] < min(times["cpu"])
    print("verdict: the device engine's median is %s the host engine's fastest run -> \"auto\" %s for runs that want the bases"
          % ("below" if verdict else "NOT below", "switches to the device engine" if verdict else "stays on the host engine (SVX_INGEST=gpu remains the way in)"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["build", "run", "ab"])
    ap.add_argument("file")
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--engine", choices=["cpu", "gpu"], default="gpu")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    {"build": build, "run": run, "ab": ab}[args.mode](args)


if __name__ == "__main__":
    main()
