"""Numbers for profiles/sort_write.txt: what svision_amd.sort writes, how small, how fast.

    python tools/sort_write_time.py [--mb 400] [--coverage 30] [--out DIR] [--tables fixed|dynamic] [--memory BYTES] [--sort-only]

  file         a synthetic HiFi sample (svision_amd.synth, one contig of --mb megabases at --coverage x, random bases), its records
               shuffled (seed 1) and written under SO:unsorted with the product's writer
  compression  sort_bam's inflated over written bytes, beside zlib at levels 1 and 6, each with Z_FIXED and with dynamic tables, on the
               SAME 0xFF00-byte blocks (the written file inflated and cut again), member overhead of 26 bytes a block included: host only
  throughput   sort_bam's seconds per stage (stats), and svx_bgzf_deflate alone on those blocks: device events, one warm-up, the
               median of 5, GB/s of input.  ingest_sort.load_sample on the same file as a yardstick
  --tables dynamic   sort_bam(tables="dynamic"); the file of tables="fixed" is written too, for the table and to compare the inflated
               bytes; svx_bgzf_deflate_dyn timed the same way beside svx_bgzf_deflate; and the phases of the dynamic kernel from
               its per-block clock readings (kernels.bgzf_deflate_dynamic(phase_ticks=True)): parse, code construction, emit as
               shares of the blocks' summed time
  --memory BYTES     sort_bam(memory_bytes=BYTES), K / M / G as the command line takes them: below the records' inflated bytes the
               file is written in spans (profiles/sort_spans.txt).  The result names the budget used, the spans and
               torch.cuda.max_memory_allocated over the timed run
  --sort-only        stop behind sort_bam's two runs: no compression table, no encoder timing, no load_sample.  With --out DIR the
               shuffled input of an earlier call with the same --mb / --coverage is taken from DIR, not made again -- several
               fresh processes time the same file
Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from svision_amd import ingest_sort, kernels, sort, synth      # noqa: E402
from svision_amd.io import bam                                  # noqa: E402
from tests import baicases, sortcases                           # noqa: E402

BLOCK = sort.BLOCK


def zlib_bytes(blocks, level, strategy):
    total = 0
    for b in blocks:
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        total += len(co.compress(b)) + len(co.flush()) + 26
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=400)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tables", choices=sort.TABLES, default="fixed")
    ap.add_argument("--memory", type=sort.parse_memory, default=None)
    ap.add_argument("--sort-only", action="store_true")
    args = ap.parse_args()
    d = args.out or tempfile.mkdtemp(prefix="sort_write_")
    shuffled = os.path.join(d, "hifi.%d.%d.shuffled.bam" % (args.mb, args.coverage))
    if not (args.sort_only and os.path.exists(shuffled)):
        make_input(args, d, shuffled)
    res = {"records": None, "input_bytes": os.path.getsize(shuffled)}
    # ---- sort_bam: stage seconds (second run: allocator and page cache warm)
    out = os.path.join(d, "hifi.sorted.bam")
    kw = {} if args.memory is None else {"memory_bytes": args.memory}
    for _ in range(2):
        stats = {}
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        sort.sort_bam(shuffled, out, stats=stats, tables=args.tables, **kw)
        wall = time.perf_counter() - t0
    res["records"] = stats["records"]
    res["sort_bam"] = dict(stats, wall_seconds=round(wall, 4), tables=args.tables, max_memory_allocated=int(torch.cuda.max_memory_allocated()),
                           device_memory_free=int(torch.cuda.mem_get_info()[0]))
    res["sort_bam"].pop("range_records", None)
    if args.sort_only:
        print(json.dumps(res))
        return
    rest(args, d, shuffled, out, res)


def make_input(args, d, shuffled):
    table, _g, _ = synth.simulate(synth.SimConfig(contigs=[("c1", args.mb * 1_000_000)], coverage=args.coverage, seed=4), with_genome=False)
    seg = bam.encode_reference_segment(table, seq="random", seed=1)
    sorted_in = os.path.join(d, "hifi.bam")
    bam.write_bam_segments(sorted_in, table.references, table.lengths, [seg], index=False)
    src = bam.read_bam(sorted_in, with_seq=True)
    perm = np.random.default_rng(1).permutation(len(src))
    bam.write_bam(shuffled, sortcases.reorder_table(src, perm, sortcases.retitled(src.header_text, "unsorted")), with_seq=True, index=False)


def rest(args, d, shuffled, out, res):
    # ---- compression on the same blocks
    stream = b"".join(data for _c, data in baicases.bgzf_blocks(open(out, "rb").read()))
    blocks = [stream[at:at + BLOCK] for at in range(0, len(stream), BLOCK)]
    n_in = len(stream)
    table_c = {"device_%s_greedy" % args.tables: os.path.getsize(out)}
    if args.tables == "dynamic":
        fixed_out = os.path.join(d, "hifi.sorted.fixed.bam")
        sort.sort_bam(shuffled, fixed_out)
        assert b"".join(data for _c, data in baicases.bgzf_blocks(open(fixed_out, "rb").read())) == stream
        table_c["device_fixed_greedy"] = os.path.getsize(fixed_out)
    for level in (1, 6):
        table_c["zlib_%d_fixed" % level] = zlib_bytes(blocks, level, zlib.Z_FIXED)
        table_c["zlib_%d_dynamic" % level] = zlib_bytes(blocks, level, zlib.Z_DEFAULT_STRATEGY)
    res["compression"] = {k: {"bytes": v, "ratio": round(n_in / v, 4)} for k, v in table_c.items()}
    res["inflated_bytes"] = n_in
    # ---- the encoder alone
    dev = torch.device("cuda", torch.cuda.current_device())
    d_in = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).to(dev)
    off = np.minimum(np.arange(len(blocks) + 1, dtype=np.int64) * BLOCK, n_in)
    d_off = torch.from_numpy(off).to(dev)
    encoders = [("deflate_kernel", kernels.bgzf_deflate)] + ([("deflate_dyn_kernel", kernels.bgzf_deflate_dynamic)] if args.tables == "dynamic" else [])
    for key, encoder in encoders:
        ms = []
        for i in range(6):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            encoder(d_in, d_off)
            b.record()
            b.synchronize()
            if i:
                ms.append(a.elapsed_time(b))
        res[key] = {"blocks": len(blocks), "ms_median_of_5": round(statistics.median(ms), 3), "ms": [round(v, 3) for v in ms],
                    "gb_per_s_of_input": round(n_in / statistics.median(ms) / 1e6, 2)}
    if args.tables == "dynamic":
        # the kernel's phases: per block the clock at its start, after the parse, after the code construction, at its end
        _s, _l, btype, ticks = kernels.bgzf_deflate_dynamic(d_in, d_off, phase_ticks=True)
        t = ticks.cpu().numpy().astype(np.float64)
        parse, codes, emit = (t[:, 1] - t[:, 0]).sum(), (t[:, 2] - t[:, 1]).sum(), (t[:, 3] - t[:, 2]).sum()
        whole = parse + codes + emit
        res["deflate_dyn_phases"] = {"parse_share": round(parse / whole, 4), "code_construction_share": round(codes / whole, 4),
                                     "emit_share": round(emit / whole, 4), "ticks_a_block_median": [float(np.median(t[:, k + 1] - t[:, k])) for k in range(3)],
                                     "block_types": [int((btype == k).sum()) for k in range(3)]}
    # ---- the yardstick: the resident sample of the same file
    fasta = bam.Fasta(sequences={"c1": b"ACGT"})
    for _ in range(2):
        st = {}
        t0 = time.perf_counter()
        ingest_sort.load_sample(shuffled, fasta, 50, stats=st)
        wall = time.perf_counter() - t0
    res["load_sample"] = {"wall_seconds": round(wall, 4), "seconds": st["seconds"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
