"""Numbers for profiles/sort_merge.txt: several inputs merged by svision_amd.sort against one file with the same records.

    python tools/sort_merge_time.py --out DIR --prepare [--retag-only] [--mb 16] [--coverage 30]
    python tools/sort_merge_time.py --out DIR --mode one|same|permuted|mixed|collide|distinct [--mb 16] [--coverage 30] [--runs 1]

  --prepare    the shuffled HiFi-shaped sample of tools/sort_write_time.py (DIR/hifi.MB.COV.shuffled.bam, the file that tool's
               --sort-only --out DIR takes too: the parent commit is timed with it on the same bytes), and from it
                 one.bam           the records as the four parts hold them, one part after the other: what a merge must equal
                 same.K.bam        four parts, the records dealt round-robin, all under the sample's header
                 permuted.K.bam    the same parts; parts 1 and 3 list a decoy contig in front of the sample's, so their records'
                                   reference indices are not the merged dictionary's: svx_record_retid on every record of them
                 mixed.K.sam       parts 1 and 3 as SAM text (part 3 without a header), for a run of BAM + SAM
                 collide.K.bam     the same parts, every record with RG:Z:1 and PG:Z:aln behind its fields, every part with its own
                                   ``@RG ID:1 PU:cell<K>`` and ``@PG ID:aln CL:...<K>`` line: under retag parts 1 .. 3 are renamed and
                                   every record of them is rewritten (svx_record_retag_measure / svx_record_retag_write)
                 distinct.K.bam    the same with the IDs ``c<K>`` / ``aln<K>`` in header and records: nothing collides
               (--retag-only: the sample, same.K, collide.K and distinct.K alone: what the modes same, collide and distinct take)
               and prints the optional fields per record of collide.0.bam (min, median, max): what a lane per record would walk
  --mode       ONE timed configuration in this process -- a warm-up run, then --runs timed ones: wall seconds, the stage seconds
               of the last run, the share of the ``retid`` stage, and a SHA-256 of the two files (one, same and mixed must print the same;
               permuted has the decoy's @SQ line and an empty reference in its index besides)
                 one        sort_bam(one.bam): the single-input path on this tree
                 same       sort_bam([same.0 .. same.3])
                 permuted   sort_bam([permuted.0 .. permuted.3])
                 mixed      sort_bam([same.0, mixed.1.sam, same.2, mixed.3.sam]): room is known behind the key passes only, the BAM parts
                            are read a second time
                 collide    sort_bam([collide.0 .. collide.3], retag=True): three inputs renamed, their records rewritten, every BAM
                            part read a second time; ``retag_share`` is the stage's share of the stage seconds
                 distinct   sort_bam([distinct.0 .. distinct.3], retag=True): the same records, nothing to rename, one read -- the
                            difference to collide is what the renames cost, the second read included
Prints one JSON object.  Fresh processes, alternating between the trees and the modes, are the caller's loop."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from svision_amd import sort                                    # noqa: E402
from svision_amd.io import bam                                  # noqa: E402
from tests import mergecases, retagcases, samtext, sortcases     # noqa: E402

PARTS = 4
DECOY = ("decoy_in_front", 12345)


def _with_decoy(table):
    """The table under a dictionary that lists a decoy contig first: every reference index one higher."""
    return bam.AlignmentTable([DECOY[0]] + list(table.references), [DECOY[1]] + list(table.lengths), np.where(table.tid >= 0, table.tid + 1, table.tid).astype(table.tid.dtype),
                              table.pos, table.flag, table.mapq, table.l_seq, table.name_id, table.names, table.cigar, table.cig_off, table.header_text.replace(
                                  "@SQ\t", "@SQ\tSN:%s\tLN:%d\n@SQ\t" % DECOY, 1), table.seq_packed, table.seq_off)


def prepare(args, d, shuffled):
    import sort_write_time
    if not os.path.exists(shuffled):
        sort_write_time.make_input(args, d, shuffled)
    src = bam.read_bam(shuffled, with_seq=True)
    rows = [np.arange(k, len(src), PARTS) for k in range(PARTS)]
    if not args.retag_only:
        bam.write_bam(os.path.join(d, "one.bam"), sortcases.reorder_table(src, np.concatenate(rows)), with_seq=True, index=False)
    refs = list(zip(src.references, src.lengths))
    for k in range(PARTS):
        part = sortcases.reorder_table(src, rows[k])
        bam.write_bam(os.path.join(d, "same.%d.bam" % k), part, with_seq=True, index=False)
        if args.retag_only:
            continue
        bam.write_bam(os.path.join(d, "permuted.%d.bam" % k), _with_decoy(part) if k % 2 else part, with_seq=True, index=False)
        if k % 2:
            with open(os.path.join(d, "mixed.%d.sam" % k), "wb") as f:
                f.write(samtext.text(refs, samtext.records_of_table(part), header="" if k == 3 else src.header_text))
    fields = []
    for k in range(PARTS):                                      # the parts' record bytes with the two tags behind them, under headers of their own
        text, part_refs, records = mergecases.raw_bam(os.path.join(d, "same.%d.bam" % k))
        for name, rg, pg in (("collide", "1", "aln"), ("distinct", "c%d" % k, "aln%d" % k)):
            tags = retagcases.z("RG", rg.encode()) + retagcases.z("PG", pg.encode())
            lines = "@RG\tID:%s\tSM:sample\tPU:cell%d\n@PG\tID:%s\tPN:aln\tCL:aln cell%d.fq\n" % (rg, k, pg, k)
            tagged = [retagcases.with_fields(r, tags) for r in records]
            mergecases.write_raw_bam(os.path.join(d, "%s.%d.bam" % (name, k)), text + lines, part_refs, tagged)
            if name == "collide" and k == 0:
                fields = sorted(retagcases.count_fields(r) for r in tagged)
        del records, tagged
    print(json.dumps({"prepared": d, "records": len(src), "fields_per_record": {"min": fields[0], "median": fields[len(fields) // 2], "max": fields[-1]}, "bytes": {n: os.path.getsize(os.path.join(d, n)) for n in sorted(os.listdir(d))}}))


def inputs_of(mode, d):
    if mode == "one":
        return os.path.join(d, "one.bam")
    if mode == "mixed":
        return [os.path.join(d, "mixed.%d.sam" % k if k % 2 else "same.%d.bam" % k) for k in range(PARTS)]
    return [os.path.join(d, "%s.%d.bam" % (mode, k)) for k in range(PARTS)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=16)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--out", required=True)
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--retag-only", action="store_true")
    ap.add_argument("--mode", choices=("one", "same", "permuted", "mixed", "collide", "distinct"), default=None)
    ap.add_argument("--runs", type=int, default=1)
    ap.add_argument("--tables", choices=sort.TABLES, default="fixed")
    args = ap.parse_args()
    d = args.out
    os.makedirs(d, exist_ok=True)
    if args.prepare:
        prepare(args, d, os.path.join(d, "hifi.%d.%d.shuffled.bam" % (args.mb, args.coverage)))
    if args.mode is None:
        return
    out = os.path.join(d, "merged.%s.%d.bam" % (args.mode, os.getpid()))
    walls = []
    for i in range(args.runs + 1):                              # (the first run warms the allocator and the page cache)
        stats = {}
        t0 = time.perf_counter()
        sort.sort_bam(inputs_of(args.mode, d), out, stats=stats, tables=args.tables, **(dict(retag=True) if args.mode in ("collide", "distinct") else {}))
        if i:
            walls.append(round(time.perf_counter() - t0, 4))
    seconds = stats["seconds"]
    digest = hashlib.sha256(open(out, "rb").read() + open(out + ".bai", "rb").read()).hexdigest()
    # (the permuted parts add the decoy's @SQ line and an empty reference to the index: another header, the same records)
    os.unlink(out)
    os.unlink(out + ".bai")
    print(json.dumps({"mode": args.mode, "wall_seconds": walls, "records": stats["records"], "inputs": stats.get("inputs"),
                      "input_records": stats.get("input_records"), "retid_inputs": stats.get("retid_inputs"), "ranges": stats["ranges"],
                      "spans": stats["spans"], "stream_bytes": stats["stream_bytes"], "seconds": seconds,
                      "retid_share": round(seconds.get("retid", 0.0) / max(sum(seconds.values()), 1e-9), 6),
                      "retag_inputs": stats.get("retag_inputs"), "retag_records": stats.get("retag_records"),
                      "retag_share": round(seconds.get("retag", 0.0) / max(sum(seconds.values()), 1e-9), 6), "sha256": digest,
                      "max_memory_allocated": int(torch.cuda.max_memory_allocated())}))


if __name__ == "__main__":
    main()
