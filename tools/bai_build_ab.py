#!/usr/bin/env python
"""A BAM without a .bai: the index built on the device + the device ingest engine, against the host engine over the whole file.

    python tools/bai_build_ab.py build DIR [--windows 20] [--kind hifi|ont]
        DIR/sample.bam like bench.py's file-inclusive job (hifi: a prefix of every GRCh38 chromosome, bench.job_contigs; ont: one
        contig of --windows windows with the bench's ONT stand-in reads), its genome DIR/genome.fa, a checkpoint DIR/m.ckpt.  The
        .bai the writer makes is moved away to DIR/shipped.bai: nothing lies next to the BAM.
    python tools/bai_build_ab.py index DIR [--runs 2]
        svision_amd.index.build_index alone, in this process (HIP context and libsvx.so up before the clock starts): total and the
        per-range split -- read, upload, inflate (tokens + LZ), crc, find_starts, walk, scan, read_back, assembly.  One JSON line a run.
    python tools/bai_build_ab.py cli DIR --mode plain|build|shipped [--root TREE]
        ONE ./SVision run of TREE (default: this tree) on DIR/sample.bam in a fresh process, wall time of the process.  plain: as it
        is (no index: host engine); build: SVX_BUILD_INDEX=1; shipped: with DIR/shipped.bai passed through a link next to a link of
        the BAM (the device engine without the build, for reference).
    python tools/bai_build_ab.py ab DIR [--runs 3] [--parent TREE]
        plain (of --parent where given: the parent commit's tree) and build alternately, and the verdict: the switch pays where the
        MEDIAN of build is below the FASTEST plain run.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build(args):
    import multiprocessing as mp
    import bench                                            # (job_contigs / _simulate_contig / random_weights: the file is built the bench's way)
    from svision_amd.io import bam
    from svision_amd.network import tf_checkpoint as ck
    os.makedirs(args.dir, exist_ok=True)
    if args.kind == "ont":
        contigs = [("chr21", args.windows * bench.WINDOW)]
    else:
        contigs = bench.job_contigs(args.windows)
    jobs = [dict(name=n, length=l, coverage=args.coverage, seed=100 + i, kind="ont" if args.kind == "ont" else None, e2e=(i, l)) for i, (n, l) in enumerate(contigs)]
    pool = mp.get_context("fork").Pool(min(len(jobs), args.procs))
    try:
        made = pool.map(bench._simulate_contig, jobs, chunksize=1)
    finally:
        pool.close()
        pool.join()
    path = os.path.join(args.dir, "sample.bam")
    bam.write_bam_segments(path, [n for n, _l in contigs], [l for _n, l in contigs], [seg for _t, _g, seg in made], index=True)
    os.replace(path + ".bai", os.path.join(args.dir, "shipped.bai"))
    bam.write_fasta(os.path.join(args.dir, "genome.fa"), {n: g for (n, _l), (_t, g, _s) in zip(contigs, made)})
    ck.write_checkpoint(os.path.join(args.dir, "m.ckpt"), bench.random_weights(0))
    print("built %s: %d windows, %d records, %.2f GB, %.2f GB inflated" % (path, sum(len(bench.windows_of(n, l)) for n, l in contigs), sum(len(t) for t, _g, _s in made),
                                                                          os.path.getsize(path) / 1e9, sum(s["inflated"] for _t, _g, s in made) / 1e9), flush=True)


def index_alone(args):
    import torch
    from svision_amd import _lib, index
    torch.zeros(1, device="cuda:0").add_(1).cpu()           # the HIP context, a first kernel, a first read-back
    _lib.load()
    path = os.path.join(args.dir, "sample.bam")
    for run in range(args.runs):
        stats = {}
        out = os.path.join(args.dir, "alone.bai")
        t0 = time.perf_counter()
        index.build_index(path, out, stats=stats)
        wall = time.perf_counter() - t0
        os.unlink(out)
        print(json.dumps({"run": run, "wall_s": round(wall, 3), "ranges": stats["ranges"], "blocks": stats["blocks"], "records": stats["records"],
                          "seconds": {k: round(v, 4) for k, v in stats["seconds"].items()}}), flush=True)
        for i, r in enumerate(stats["per_range"]):
            print(json.dumps({"run": run, "range": i, **{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}}), flush=True)


def cli_once(args, mode=None, root=None):
    mode, root = mode or args.mode, os.path.abspath(root or args.root or ROOT)
    d = args.dir
    out = os.path.join(d, "out_%s" % mode)
    shutil.rmtree(out, ignore_errors=True)
    bam_path = os.path.join(d, "sample.bam")
    env = {k: v for k, v in os.environ.items() if k not in ("SVX_BUILD_INDEX", "SVX_INGEST")}
    env.update(PYTHONPATH=root, SVX_TIMING="1")
    if mode == "build":
        env["SVX_BUILD_INDEX"] = "1"
    if mode == "shipped":
        os.makedirs(os.path.join(d, "with_index"), exist_ok=True)
        for src, dst in ((bam_path, "sample.bam"), (os.path.join(d, "shipped.bai"), "sample.bam.bai")):
            if not os.path.exists(os.path.join(d, "with_index", dst)):
                os.symlink(src, os.path.join(d, "with_index", dst))
        bam_path = os.path.join(d, "with_index", "sample.bam")
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(root, "SVision"), "-o", out, "-b", bam_path, "-m", os.path.join(d, "m.ckpt"), "-g", os.path.join(d, "genome.fa"),
                        "-n", "S", "-s", "5", "--batch_size", "64", "-t", str(args.threads)], capture_output=True, text=True, env=env, timeout=1500)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        print(r.stdout[-3000:] + r.stderr[-3000:])
        raise SystemExit("the %s run failed" % mode)
    engine = "gpu" if "'engine': 'gpu'" in r.stdout else "cpu" if "'engine': 'cpu'" in r.stdout else "?"
    vcf = open(os.path.join(out, "S.svision.s5.vcf")).read()
    built = next((float(l.split()[-2]) for l in r.stdout.splitlines() if l.startswith("index built on the device")), None)
    res = {"mode": mode, "tree": os.path.relpath(root, ROOT), "wall_s": round(wall, 3), "engine": engine, "index_s": built, "vcf_records": sum(1 for l in vcf.splitlines() if not l.startswith("#")),
           "vcf_crc32": zlib.crc32(vcf.encode())}
    print(json.dumps(res), flush=True)
    return res


def ab(args):
    plain, built = [], []
    for _ in range(args.runs):
        plain.append(cli_once(args, "plain", args.parent or ROOT))
        built.append(cli_once(args, "build", ROOT))
    a, b = sorted(r["wall_s"] for r in plain), sorted(r["wall_s"] for r in built)
    same = len({r["vcf_crc32"] for r in plain + built}) == 1
    print(json.dumps({"plain_s": a, "build_s": b, "fastest_plain_s": a[0], "median_build_s": b[len(b) // 2], "switch_pays": b[len(b) // 2] < a[0], "same_vcf": same,
                      "engines": sorted({r["engine"] for r in plain}) + sorted({r["engine"] for r in built})}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("build", "index", "cli", "ab"))
    ap.add_argument("dir")
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--kind", choices=("hifi", "ont"), default="hifi")
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--runs", type=int, default=None)
    ap.add_argument("--mode", choices=("plain", "build", "shipped"), default="plain")
    ap.add_argument("--root", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--threads", type=int, default=8, help="-t of the SVision runs")
    args = ap.parse_args()
    if args.runs is None:
        args.runs = 3 if args.what == "ab" else 2
    {"build": build, "index": index_alone, "cli": cli_once, "ab": ab}[args.what](args)


if __name__ == "__main__":
    main()
