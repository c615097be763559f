"""Numbers for profiles/sort_sam.txt: sort_bam on an aligner's SAM text against sort_bam on the same records as an unsorted BAM.

    python tools/sort_sam_time.py --shape hifi|ont [--mb 40] [--coverage 30] [--out DIR] [--runs 3] [--once sam|bam] [--chunks]
                                  [--pipe [--memory BYTES]]

  files     a synthetic sample (svision_amd.synth: one contig of --mb megabases at --coverage x; ``ont``: log-normal read lengths, 6 %
            small events), its records shuffled (seed 1), random bases and phred values, NM:i and rq:f on every read and an MM:Z / ML:B:C
            pair on every 8th, written as SAM text; the unsorted BAM of the same records: io.sam.read_sam's records behind the same
            header, in BGZF blocks of zlib level 1 (tests/baicases.write_stream)
  runs      --runs times sort_bam(text) and sort_bam(BAM), alternating, after one warm-up of each; the two outputs compared byte for
            byte.  Stage seconds are index._Clock's: a host clock, the device drained at every boundary
  rates     text bytes over the seconds of the stages lines, measure, encode and read of the text runs
  host      io.sam.encode_line on the first 10,000 lines: what a line that the kernels leave to the host costs
  --chunks  sort_bam(text) once more at range_bytes of 16, 64 and 256 MB
  --once    ONE sort_bam of the text or the BAM and nothing else (files of an earlier call with the same --out are taken): the run a
            kernel trace is taken of
  --pipe    numbers for profiles/sort_pipe.txt instead: the same text three ways, alternating, --runs times after one warm-up of each --
            as a file, through ``cat`` (sort_bam reads /dev/fd/N: one pass, the records kept in core) and through ``cat`` under a budget
            of --memory bytes (default: a fifth of the records' bytes), which spools; wall and stage seconds, what the reader thread
            waited for, how many times the stream grew, and whether the three outputs are identical
Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from svision_amd import sort, synth                             # noqa: E402
from svision_amd.io import sam                                  # noqa: E402
from tests import baicases                                      # noqa: E402

OPS = np.frombuffer(b"MIDNSHP=X", np.uint8)


def write_text(path, shape, mb, coverage):
    cfg = synth.SimConfig(contigs=[("c1", mb * 1_000_000)], coverage=coverage, seed=4)
    if shape == "ont":
        cfg.lognormal, cfg.read_len_mean, cfg.err_rate = True, 20_000.0, 0.06
    table, _g, _s = synth.simulate(cfg, with_genome=False)
    rng = np.random.default_rng(1)
    bases = np.frombuffer(b"ACGT", np.uint8)
    with open(path, "wb") as f:
        f.write(b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c1\tLN:%d\n@PG\tID:synth\tPN:synth\n" % (mb * 1_000_000))
        for i in rng.permutation(len(table.tid)):
            words = table.cigar[int(table.cig_off[i]):int(table.cig_off[i + 1])]
            cigar = "".join("%d%s" % (w >> 4, "MIDNSHP=X"[w & 15]) for w in words.tolist())
            n = int(sum(w >> 4 for w in words.tolist() if (w & 15) in (0, 1, 4, 7, 8)))
            cols = [table.names[int(table.name_id[i])], str(int(table.flag[i])), "c1", str(int(table.pos[i]) + 1), str(int(table.mapq[i])), cigar, "*", "0",
                    "0", bases[rng.integers(0, 4, n)].tobytes().decode(), (rng.integers(0, 60, n, dtype=np.uint8) + 33).tobytes().decode(),
                    "NM:i:%d" % (int(i) % 3000), "rq:f:0.%04d" % (int(i) * 7919 % 10000)]
            if i % 8 == 0:
                k = n // 40
                cols += ["MM:Z:C+m?" + "".join(",%d" % v for v in rng.integers(0, 30, k)) + ";", "ML:B:C" + "".join(",%d" % v for v in rng.integers(0, 256, k))]
            f.write("\t".join(cols).encode() + b"\n")


def timed(path, out, **kw):
    stats = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sort.sort_bam(path, out, stats=stats, **kw)
    stats["wall_seconds"] = round(time.perf_counter() - t0, 4)
    stats.pop("range_records", None)
    return stats


def timed_pipe(text, out, **kw):
    """sort_bam on the text as ``cat`` writes it into a pipe."""
    import subprocess
    with subprocess.Popen(["cat", text], stdout=subprocess.PIPE) as cat:
        try:
            return timed("/dev/fd/%d" % cat.stdout.fileno(), out, **kw)
        finally:
            cat.stdout.close()
            cat.wait()


def pipe_runs(text, d, runs, memory):
    outs = {w: os.path.join(d, "pipe_%s.bam" % w) for w in ("file", "in_core", "spooled")}
    got = {w: [] for w in outs}
    for r in range(runs + 1):
        st = timed(text, outs["file"])
        budget = memory or max((st["stream_bytes"] - 4) // 5, 1)
        for w, one in (("file", st), ("in_core", timed_pipe(text, outs["in_core"])), ("spooled", timed_pipe(text, outs["spooled"], memory_bytes=budget))):
            if r:
                got[w].append(one)
    res = {"memory_bytes_spooled": budget,
           "outputs_identical": all(open(outs["file"] + e, "rb").read() == open(outs[w] + e, "rb").read() for w in ("in_core", "spooled") for e in ("", ".bai"))}
    for w, sts in got.items():
        stages = sorted({k for st in sts for k, v in st["seconds"].items() if v > 0})
        res[w] = {"wall_seconds": [st["wall_seconds"] for st in sts], "seconds": {k: [st["seconds"][k] for st in sts] for k in stages},
                  "records": sts[0]["records"], "ranges": sts[0]["ranges"], "spans": sts[0]["spans"], "stream_bytes": sts[0]["stream_bytes"],
                  "pipe": [st.get("pipe") for st in sts]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("hifi", "ont"), default="hifi")
    ap.add_argument("--mb", type=int, default=40)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--once", choices=("sam", "bam"), default=None)
    ap.add_argument("--chunks", action="store_true")
    ap.add_argument("--pipe", action="store_true")
    ap.add_argument("--memory", type=sort.parse_memory, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sort_sam_time.py measures on the GPU; there is none")
    d = args.out or tempfile.mkdtemp(prefix="sort_sam_")
    os.makedirs(d, exist_ok=True)
    text = os.path.join(d, "%s.%d.%d.sam" % (args.shape, args.mb, args.coverage))
    unsorted = text[:-4] + ".unsorted.bam"
    res = {"shape": args.shape}
    if args.pipe:
        if not os.path.exists(text):
            write_text(text, args.shape, args.mb, args.coverage)
        res.update(text_bytes=os.path.getsize(text), **pipe_runs(text, d, args.runs, args.memory))
        print(json.dumps(res))
        return
    if not (os.path.exists(text) and os.path.exists(unsorted)):
        write_text(text, args.shape, args.mb, args.coverage)
        t0 = time.perf_counter()
        head, records = sam.read_sam(text)
        res["read_sam_seconds"] = round(time.perf_counter() - t0, 3)
        baicases.write_stream(unsorted, sam.bam_header_bytes(head) + b"".join(records), level=1)
        del records
    res.update(text_bytes=os.path.getsize(text), bam_bytes=os.path.getsize(unsorted))
    outs = {"sam": os.path.join(d, "from_sam.bam"), "bam": os.path.join(d, "from_bam.bam")}
    paths = {"sam": text, "bam": unsorted}
    if args.once:
        res[args.once] = timed(paths[args.once], outs[args.once])
        print(json.dumps(res))
        return
    # ---- the host's rate
    tid_of = {b"c1": 0}
    with open(text, "rb") as f:
        lines = [l.rstrip(b"\n") for l in f if not l.startswith(b"@")][:10000]
    t0 = time.perf_counter()
    n_bytes = sum(len(sam.encode_line(l, tid_of)) for l in lines)
    dt = time.perf_counter() - t0
    res["host_encode"] = {"lines": len(lines), "seconds": round(dt, 3), "lines_per_s": round(len(lines) / dt, 1),
                          "text_mb_per_s": round(sum(map(len, lines)) / dt / 1e6, 2), "record_bytes": n_bytes}
    # ---- alternating runs, one warm-up of each
    runs = {"sam": [], "bam": []}
    for r in range(args.runs + 1):
        for what in ("sam", "bam"):
            st = timed(paths[what], outs[what])
            if r:
                runs[what].append(st)
    same = all(open(outs["sam"] + e, "rb").read() == open(outs["bam"] + e, "rb").read() for e in ("", ".bai"))
    res["outputs_identical"] = same
    for what in ("sam", "bam"):
        stages = sorted({k for st in runs[what] for k, v in st["seconds"].items() if v > 0})
        res[what] = {"wall_seconds": [st["wall_seconds"] for st in runs[what]],
                     "seconds": {k: [st["seconds"][k] for st in runs[what]] for k in stages},
                     "records": runs[what][0]["records"], "ranges": runs[what][0]["ranges"], "spans": runs[what][0]["spans"],
                     "inflated_bytes": runs[what][0]["inflated_bytes"], "host_lines": runs[what][0].get("host_lines")}
    med = {k: statistics.median(v) for k, v in res["sam"]["seconds"].items()}
    res["sam_rates_gb_per_s_of_text"] = {k: round(res["text_bytes"] / med[k] / 1e9, 3) for k in ("read", "upload", "lines", "measure", "encode") if med.get(k)}
    if args.chunks:
        res["chunks"] = {}
        for mbytes in (16, 64, 256):
            st = timed(text, outs["sam"], range_bytes=mbytes << 20)
            res["chunks"][str(mbytes)] = {"wall_seconds": st["wall_seconds"], "ranges": st["ranges"],
                                          "front_end_seconds": round(sum(st["seconds"][k] for k in ("read", "upload", "lines", "measure", "encode", "read_back", "host_lines", "keep")), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
