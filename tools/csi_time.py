#!/usr/bin/env python
"""What the looser bounds of a ``.csi`` cost the device ingest engine: the same file read through its ``.bai`` and through its ``.csi``.

    python tools/csi_time.py build FILE.bam [--contigs 8] [--length 2000000] [--coverage 30]
        a HiFi-shaped file of svision_amd.synth -- simulated reads on ``--contigs`` references of ``--length`` bases, random bases and
        qualities, 64 KB blocks (encode_reference_segment) -- with the writer's .bai, the .csi built on the device beside it
        (svision_amd.index.build_index) and FILE.bam.json (the windows)
    python tools/csi_time.py run FILE.bam --index bai|csi
        ONE pass in this process: a ChromosomeFeed on the device engine over the file's windows, in slices of about --slice-mb
        compressed megabytes; timed from opening the index to the last hand-over.  The HIP context and libsvx.so are up before the
        clock starts.  Prints one JSON line: the decoder's seconds per stage, the slices, the cuts that had to be made again, and
        per slice the compressed bytes its file range spans.
    python tools/csi_time.py ab FILE.bam [--runs 3]
        `run` through the .bai and the .csi alternately, a fresh process each, then the medians side by side and, slice by slice,
        how many more bytes the .csi plan reads on either end.

Reported, not gated: the reference of the comparison is the .bai road of the same run.
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

WINDOW = 500_000
STAGES = ("read_s", "h2d_inflate_s", "walk_s", "d2h_s", "names_s")


def _simulate(job):
    import numpy as np                                      # noqa: F401
    from svision_amd import synth
    from svision_amd.io import bam
    name, length, coverage, seed, tid = job
    table, _genome, _svs = synth.simulate(synth.SimConfig(contigs=[(name, length)], coverage=coverage, seed=seed), with_genome=False)
    table.tid[:] = tid
    return len(table), bam.encode_reference_segment(table, seq="random", seed=seed)


def build(args):
    import multiprocessing as mp
    from svision_amd import index
    from svision_amd.io import bam
    contigs = [("chr%d" % (i + 1), args.length) for i in range(args.contigs)]
    pool = mp.get_context("fork").Pool(min(len(contigs), args.procs))
    try:
        made = pool.map(_simulate, [(n, l, args.coverage, 300 + i, i) for i, (n, l) in enumerate(contigs)], chunksize=1)
    finally:
        pool.close()
        pool.join()
    bam.write_bam_segments(args.file, [n for n, _l in contigs], [l for _n, l in contigs], [seg for _n, seg in made])
    stats = {}
    index.build_index(args.file, args.file + ".csi", fmt="csi", stats=stats)
    windows = [(n, a, min(l, a + WINDOW)) for n, l in contigs for a in range(0, l, WINDOW)]
    with open(args.file + ".json", "w") as f:
        json.dump({"windows": windows, "records": int(sum(n for n, _s in made))}, f)
    print("built %s: %d records, %d windows, %.1f MB; .bai %d bytes, .csi %d bytes (built in %.2f s)"
          % (args.file, sum(n for n, _s in made), len(windows), os.path.getsize(args.file) / 1e6, os.path.getsize(args.file + ".bai"),
             os.path.getsize(args.file + ".csi"), sum(stats["seconds"].values())))


def run(args):
    import types
    import torch
    from svision_amd import _lib, ingest, ingest_gpu
    from svision_amd.io import bam
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev).add_(1).cpu()               # the HIP context, a first kernel, a first read-back
    _lib.load()
    os.environ["SVX_SLICE_BYTES"] = str(args.slice_mb << 20)
    with open(args.file + ".json") as f:
        meta = json.load(f)
    tasks = {}
    for c, a, b in meta["windows"]:
        tasks.setdefault(c, []).append((a, b))
    opts = types.SimpleNamespace(hash=False, graph=False, contig=False, min_sv_size=50)
    head = bam.read_bam_header(args.file)
    chroms = [c for c in head.references if c in tasks]
    t0 = time.perf_counter()
    feed = ingest.ChromosomeFeed(args.file, bam.Fasta(sequences={}), opts, chroms, head.references, head.lengths, device=dev,
                                 index=args.file + "." + args.index, threads=ingest.decode_threads(), engine="gpu", tasks=tasks)
    try:
        while not feed.finished:
            feed.poll(block=True)
        seconds = time.perf_counter() - t0
        if feed.error is not None:
            raise feed.error
        records = sum(len(smp.table) for ents in feed.samples.values() for _lo, _hi, _key, smp, _m in ents)
        dec = feed.decoder
        # the plan the run was served from (no cut was made again: the same call gives the same units)
        tids = [head.references.index(c) for c in chroms]
        units = dec.plan_units(tids, lambda t: tasks.get(head.references[t]), dec.estimate_reach(tids))
        d = feed.stats.get("device_decoder", {})
        print(json.dumps({"index": args.index, "engine": feed.stats["engine"], "seconds": round(seconds, 4), "slices": int(feed.stats["slices"]),
                          "replans": int(feed.stats["replans"]), "records": records, "margin": dec.estimate_reach(tids),
                          "stages": {k: d.get(k) for k in STAGES}, "bytes_in": d.get("bytes_in"), "blocks": d.get("blocks"),
                          "slice_bytes": [ingest_gpu._size_of(u) for u in units],
                          "slice_ends": [[u.tid, u.lo, u.hi, u.vlo >> 16, u.vhi >> 16] for u in units]}))
    finally:
        feed.close()


def ab(args):
    lines = {"bai": [], "csi": []}
    for i in range(args.runs):
        for kind in ("bai", "csi"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "run", args.file, "--index", kind, "--slice-mb", str(args.slice_mb)],
                               capture_output=True, text=True, timeout=args.timeout)
            if r.returncode != 0:                              # nothing more is started behind a failed run
                sys.stdout.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit("run %d, index %s: exit status %d" % (i + 1, kind, r.returncode))
            line = json.loads(r.stdout.strip().splitlines()[-1])
            assert line["engine"] == "gpu" and line["index"] == kind, line
            lines[kind].append(line)
            print("run %d  %s" % (i + 1, json.dumps({k: v for k, v in line.items() if k not in ("slice_bytes", "slice_ends")})), flush=True)

    def med(kind, get):
        v = sorted(get(l) for l in lines[kind])
        return v[len(v) // 2]
    print("%-16s %10s %10s" % ("median of %d" % args.runs, ".bai", ".csi"))
    print("%-16s %10.4f %10.4f" % ("seconds", med("bai", lambda l: l["seconds"]), med("csi", lambda l: l["seconds"])))
    for k in STAGES:
        print("%-16s %10.4f %10.4f" % (k, med("bai", lambda l: l["stages"][k] or 0.0), med("csi", lambda l: l["stages"][k] or 0.0)))
    a, b = lines["bai"][0], lines["csi"][0]
    print("%-16s %10d %10d" % ("bytes_in", a["bytes_in"], b["bytes_in"]))
    print("%-16s %10d %10d" % ("slices", a["slices"], b["slices"]))
    print("%-16s %10d %10d" % ("replans", max(l["replans"] for l in lines["bai"]), max(l["replans"] for l in lines["csi"])))
    print("%-16s %10d %10d   (+%.2f %%)" % ("sum slice bytes", sum(a["slice_bytes"]), sum(b["slice_bytes"]),
                                           100.0 * (sum(b["slice_bytes"]) - sum(a["slice_bytes"])) / max(sum(a["slice_bytes"]), 1)))
    if [e[:3] for e in a["slice_ends"]] == [e[:3] for e in b["slice_ends"]]:
        left = sum(max(x[3] - y[3], 0) for x, y in zip(a["slice_ends"], b["slice_ends"]))
        right = sum(max(y[4] - x[4], 0) for x, y in zip(a["slice_ends"], b["slice_ends"]))
        print("the same %d slices by windows; the .csi plan begins %d bytes earlier in all (from_voff: a bin's loffset instead of the 16 kb "
              "window's entry) and ends %d bytes later in all (to_voff: the next bin that has a chunk of its own)" % (len(a["slice_ends"]), left, right))
        print("per slice, compressed bytes .bai / .csi: " + " ".join("%d/%d" % (x, y) for x, y in zip(a["slice_bytes"], b["slice_bytes"])))
    else:
        print("the two plans cut different slices: %d and %d" % (len(a["slice_ends"]), len(b["slice_ends"])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["build", "run", "ab"])
    ap.add_argument("file")
    ap.add_argument("--contigs", type=int, default=8)
    ap.add_argument("--length", type=int, default=2_000_000)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--procs", type=int, default=14)
    ap.add_argument("--index", choices=["bai", "csi"], default="csi")
    ap.add_argument("--slice-mb", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    args = ap.parse_args()
    {"build": build, "run": run, "ab": ab}[args.mode](args)


if __name__ == "__main__":
    main()
