"""Numbers for profiles/device_sort_inputs.txt: ingest_sort.load_sample on an aligner's text, a pipe and an unsorted BAM, beside
sort_bam and the read of the file it writes; and the pack kernels alone beside the kernels the text would otherwise go through.

    python tools/device_sort_inputs_time.py --shape hifi|ont [--mb MB] [--coverage 30] [--out DIR] [--runs 2] [--chunk-mb 64] [--read feed|host]

  files     tools/sort_sam_time.py's: a synthetic sample (svision_amd.synth: one contig of --mb megabases at --coverage x; the
            defaults, --mb 16 for hifi and 9 for ont, give about 1 GB of text; ``ont``: log-normal read lengths, 6 % small events),
            shuffled (seed 1), random bases and phred values, NM:i and rq:f on every read, MM:Z / ML:B:C on every 8th, as SAM text;
            the unsorted BAM of the same records
  roads     after one warm-up of each, --runs times, alternating: load_sample(text), load_sample(the text through ``cat``:
            /dev/fd/N), load_sample(the unsorted BAM), and sort_bam(text) followed by the pipeline's read of the file it wrote
            (ingest.ChromosomeFeed on the device engine, every reference handed over; --read host: io.bam.read_bam, the host's
            decoder, instead).  Wall seconds, and index._Clock's stage seconds -- a host clock, the device drained at every
            boundary.  The four tables are compared (the written file's through read_bam, outside the timing)
  kernels   one chunk of --chunk-mb MB of the text's lines: svx_sam_pack_count and svx_sam_pack_extract against svx_sam_measure,
            svx_sam_encode, svx_bam_walk_count and svx_bam_walk_extract (a walk start every 32 records) on the same lines -- each
            launch between two device events, one warm-up, the median of 5.  The prefix sums between the launches are the host's and
            are not timed on either side
Prints one JSON object."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from svision_amd import _lib, index, ingest, ingest_sort, kernels, sort             # noqa: E402
from svision_amd.io import bam, sam                                         # noqa: E402
from tests import baicases, sortcases                                       # noqa: E402
from tools.sort_sam_time import write_text                                  # noqa: E402

FASTA = bam.Fasta(sequences={"c1": b"ACGT"})


def loaded(src, stats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sample = ingest_sort.load_sample(src, FASTA, 50, stats=stats)
    stats["wall_seconds"] = round(time.perf_counter() - t0, 4)
    return sample


def piped(text, stats):
    with subprocess.Popen(["cat", text], stdout=subprocess.PIPE) as cat:
        try:
            return loaded("/dev/fd/%d" % cat.stdout.fileno(), stats)
        finally:
            cat.stdout.close()
            cat.wait()


def streamed(path):
    """The pipeline's read of a sorted, indexed file: ingest.ChromosomeFeed on the device engine, every reference handed over and
    released -> the records seen."""
    head = bam.read_bam_header(path)
    opts = types.SimpleNamespace(hash=False, graph=False, contig=False, min_sv_size=50)
    feed = ingest.ChromosomeFeed(path, bam.Fasta(sequences={}), opts, head.references, head.references, head.lengths,
                                 device=torch.device("cuda", torch.cuda.current_device()), index=bam.find_index(path), threads=ingest.decode_threads(),
                                 engine="gpu")
    records = 0
    try:
        for chrom in head.references:
            _key, smp = feed.get(chrom, block=True)
            records += len(smp.table)
            feed.release(chrom)
    finally:
        feed.close()
    return records


def written(text, out, stats, read):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sort.sort_bam(text, out, stats=stats)
    stats["sort_bam_wall_seconds"] = round(time.perf_counter() - t0, 4)
    table = None
    if read == "feed":
        stats["feed_records"] = streamed(out)
        torch.cuda.synchronize()
    else:
        table = bam.read_bam(out)
    stats["wall_seconds"] = round(time.perf_counter() - t0, 4)
    stats.pop("range_records", None)
    return bam.read_bam(out) if table is None else table         # (the table the roads are compared by: not timed)


def event_ms(launch):
    """One warm-up, then the median of 5 of ``launch()`` between two device events."""
    ms = []
    for i in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        if i:
            ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 3)


def kernels_alone(text, chunk_bytes):
    head = sam.parse_header(sam.header_end(text))
    at, n = sam.chunk_places(text, len(sam.header_end(text)), chunk_bytes)[0]
    with open(text, "rb") as f:
        f.seek(at)
        data = np.frombuffer(f.read(n), np.uint8)
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, st = _lib.load(), kernels._stream_ptr(dev)
    d_text = torch.zeros(n + kernels.SAM_SLACK, dtype=torch.uint8, device=dev)
    d_text[:n].copy_(torch.from_numpy(data.copy()))
    table = kernels.sam_ref_table(head.references, dev)
    line_off, n_lines = kernels.sam_lines(d_text, n)
    res = {"text_bytes": n, "lines": n_lines, "lines_ms": event_ms(lambda: kernels.sam_lines(d_text, n, n_lines + 1))}
    # ---- the pack road
    res["pack_count_ms"] = event_ms(lambda: kernels.sam_pack_count(d_text, n, line_off, n_lines, table, False))
    d_status, _fields, d_counts = kernels.sam_pack_count(d_text, n, line_off, n_lines, table, False)
    counts = d_counts.cpu().numpy().astype(np.int64)
    assert not d_status.cpu().numpy().any()
    off = np.zeros((2, n_lines + 1), np.int64)
    np.cumsum(counts[:2], axis=1, out=off[:, 1:])
    out = {"d_tid": torch.empty(n_lines, dtype=torch.int32, device=dev), "d_pos": torch.empty(n_lines, dtype=torch.int32, device=dev),
           "d_l_seq": torch.empty(n_lines, dtype=torch.int32, device=dev), "d_flag": torch.empty(n_lines, dtype=torch.int16, device=dev),
           "d_mapq": torch.empty(n_lines, dtype=torch.uint8, device=dev), "d_cigar": torch.empty(int(off[0, -1]) + 4, dtype=torch.int32, device=dev),
           "d_names": torch.empty(int(off[1, -1]) + 4, dtype=torch.uint8, device=dev)}
    res["pack_extract_ms"] = event_ms(lambda: kernels.sam_pack_extract(d_text, n, line_off, n_lines, table, d_status, list(off), out))
    res["packed_bytes"] = int(4 * off[0, -1] + off[1, -1] + 15 * n_lines)
    # ---- the road through BAM records
    res["measure_ms"] = event_ms(lambda: kernels.sam_measure(d_text, n, line_off, n_lines, table))
    d_len = kernels.sam_measure(d_text, n, line_off, n_lines, table)[0]
    length = d_len.cpu().numpy()
    res["host_lines"] = int((length < 0).sum())
    rec_off = np.concatenate([[0], np.cumsum(np.maximum(length, 0).astype(np.int64))])
    total = int(rec_off[-1])
    d_raw = torch.zeros((total + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
    d_off, d_flag1 = torch.from_numpy(rec_off[:-1].copy()).to(dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ref = (table.hash.data_ptr(), table.tid.data_ptr(), table.name_off.data_ptr(), table.names.data_ptr(), table.n)
    res["encode_ms"] = event_ms(lambda: _lib.check(lib.svx_sam_encode(d_text.data_ptr(), line_off.data_ptr(), n_lines, *ref, d_len.data_ptr(),
                                                                        d_off.data_ptr(), 0, d_raw.data_ptr(), d_flag1.data_ptr(), st), "svx_sam_encode"))
    res["record_bytes"] = total
    starts = np.unique(np.append(rec_off[:-1][length >= 0][::32], total)).astype(np.uint64)
    n_starts = int(starts.size) - 1
    d_starts = torch.from_numpy(starts.view(np.int64)).to(dev)
    d_wcounts = torch.empty((n_starts, 4), dtype=torch.int64, device=dev)
    res["walk_count_ms"] = event_ms(lambda: _lib.check(lib.svx_bam_walk_count(d_raw.data_ptr(), d_starts.data_ptr(), n_starts, d_wcounts.data_ptr(), st),
                                                       "svx_bam_walk_count"))
    wc = d_wcounts.cpu().numpy()
    assert not wc[:, 3].any()
    base = np.zeros((n_starts, 3), np.int64)
    base[1:] = np.cumsum(wc[:-1, :3], axis=0)
    n_rec, words, name_bytes = (int(v) for v in wc[:, :3].sum(axis=0))
    d_base = torch.from_numpy(base).to(dev)
    w = {"tid": torch.empty(n_rec, dtype=torch.int32, device=dev), "pos": torch.empty(n_rec, dtype=torch.int32, device=dev),
         "l_seq": torch.empty(n_rec, dtype=torch.int32, device=dev), "flag": torch.empty(n_rec, dtype=torch.int16, device=dev),
         "mapq": torch.empty(n_rec, dtype=torch.uint8, device=dev), "cig_off": torch.empty(n_rec + 1, dtype=torch.int64, device=dev),
         "name_off": torch.empty(n_rec + 1, dtype=torch.int64, device=dev), "cigar": torch.empty(words + 4, dtype=torch.int32, device=dev),
         "names": torch.empty(max(name_bytes, 1), dtype=torch.uint8, device=dev)}
    res["walk_extract_ms"] = event_ms(lambda: _lib.check(lib.svx_bam_walk_extract(
        d_raw.data_ptr(), d_starts.data_ptr(), n_starts, d_base.data_ptr(), w["tid"].data_ptr(), w["pos"].data_ptr(), w["flag"].data_ptr(),
        w["mapq"].data_ptr(), w["l_seq"].data_ptr(), w["cig_off"].data_ptr(), w["cigar"].data_ptr(), w["name_off"].data_ptr(), w["names"].data_ptr(),
        n_rec, st), "svx_bam_walk_extract"))
    taken = length >= 0
    res["same_arrays"] = bool(n_rec == int(taken.sum()) and torch.equal(w["tid"], out["d_tid"][torch.from_numpy(taken).to(dev)])
                              and words == int(counts[0][taken].sum()) and name_bytes == int(counts[1][taken].sum()))
    res["pack_ms"] = round(res["pack_count_ms"] + res["pack_extract_ms"], 3)
    res["through_records_ms"] = round(res["measure_ms"] + res["encode_ms"] + res["walk_count_ms"] + res["walk_extract_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("hifi", "ont"), default="hifi")
    ap.add_argument("--mb", type=int, default=None, help="default: 16 (hifi), 9 (ont) -- about 1 GB of text")
    ap.add_argument("--read", choices=("feed", "host"), default="feed")
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--chunk-mb", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("device_sort_inputs_time.py measures on the GPU; there is none")
    args.mb = args.mb or {"hifi": 16, "ont": 9}[args.shape]
    d = args.out or tempfile.mkdtemp(prefix="device_sort_inputs_")
    os.makedirs(d, exist_ok=True)
    text = os.path.join(d, "%s.%d.%d.sam" % (args.shape, args.mb, args.coverage))
    unsorted = text[:-4] + ".unsorted.bam"
    if not (os.path.exists(text) and os.path.exists(unsorted)):
        write_text(text, args.shape, args.mb, args.coverage)
        head, records = sam.read_sam(text)
        baicases.write_stream(unsorted, sam.bam_header_bytes(head) + b"".join(records), level=1)
        del records
    res = {"shape": args.shape, "mb": args.mb, "runs": args.runs, "read": args.read, "text_bytes": os.path.getsize(text), "bam_bytes": os.path.getsize(unsorted)}
    out = os.path.join(d, "written.bam")
    roads = (("text", lambda st: loaded(text, st).table), ("pipe", lambda st: piped(text, st).table), ("bam", lambda st: loaded(unsorted, st).table),
             ("sort_bam_and_read", lambda st: written(text, out, st, args.read)))
    runs, tables = {k: [] for k, _f in roads}, {}
    for r in range(args.runs + 1):
        for what, road in roads:
            st = {}
            tables[what] = road(st)
            if r:
                runs[what].append(st)
    same = True
    for what in ("pipe", "bam", "sort_bam_and_read"):
        try:
            sortcases.assert_same_table(tables[what], tables["text"], what=what)
        except AssertionError:
            same = False
    res["tables_identical"] = same
    for what, sts in runs.items():
        stages = sorted({k for st in sts for k, v in st["seconds"].items() if v > 0})
        res[what] = {"wall_seconds": [st["wall_seconds"] for st in sts], "seconds": {k: [st["seconds"][k] for st in sts] for k in stages},
                     "records": sts[0]["records"], "ranges": sts[0]["ranges"], "host_lines": sts[0].get("host_lines")}
        if what == "sort_bam_and_read":
            res[what]["sort_bam_wall_seconds"] = [st["sort_bam_wall_seconds"] for st in sts]
            res[what]["feed_records"] = sts[0].get("feed_records")
    res["kernels"] = kernels_alone(text, args.chunk_mb << 20)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
