"""Numbers for profiles/sort_tags.txt: svision_amd.sort with optional fields removed (--drop-tags / --keep-tags) against the same file
sorted as it is, on this tree and on the parent commit.

    python tools/sort_tags_time.py --out DIR --prepare [--mb 16] [--coverage 30]
    python tools/sort_tags_time.py --out DIR --mode off|drop|keep [--root TREE] [--mb 16] [--coverage 30] [--runs 1]

  --prepare    the shuffled HiFi-shaped sample of tools/sort_write_time.py (DIR/hifi.MB.COV.shuffled.bam) and from it
                 kinetics.bam    the same records, every one with what pbmm2 carries over from an unaligned HiFi BAM behind its fields:
                                 fi, fp, ri, rp (B:C arrays of the read's length), MM:Z and ML:B:C (a modification call every 50
                                 bases), and NM:i, RG:Z in front of them -- the fields a caller keeps
               and prints the records, their bytes and the share of them that the six added fields make up
  --mode       ONE timed configuration in this process -- a warm-up run, then --runs timed ones: wall seconds, the stage seconds of
               the last run, the share of the ``tags`` stage, inflated and written bytes, ranges and range_reads (equal: no range was
               read twice), and a SHA-256 of the two files
                 off     sort_bam(kinetics.bam): the switch off.  --root TREE: the tree whose svision_amd is timed -- a checkout of the
                         PARENT commit, built, takes this mode only
                 drop    sort_bam(kinetics.bam, drop_tags="fi,fp,ri,rp")
                 keep    sort_bam(kinetics.bam, keep_tags="RG,NM")
Prints one JSON object.  Fresh processes, alternating between the trees and the modes, are the caller's loop."""
import argparse
import hashlib
import json
import os
import struct
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP, KEEP = "fi,fp,ri,rp", "RG,NM"


def prepare(args, d, shuffled):
    import numpy as np
    import sort_write_time
    from tests import mergecases
    if not os.path.exists(shuffled):
        sort_write_time.make_input(args, d, shuffled)
    text, refs, records = mergecases.raw_bam(shuffled)
    pattern = (np.arange(1 << 20, dtype=np.int64) * 7 + 3).astype(np.uint8).tobytes()
    base = sum(len(r) for r in records)
    added = 0
    for i, r in enumerate(records):
        l_seq = struct.unpack_from("<I", r, 20)[0]
        calls = l_seq // 50
        arrays = b"".join(tag + b"BC" + struct.pack("<I", l_seq) + pattern[k:k + l_seq] for k, tag in enumerate((b"fi", b"fp", b"ri", b"rp")))
        fields = b"NMi" + struct.pack("<i", i % 97) + b"RGZmovie1\0" + arrays + b"MMZC+m?," + b"49," * calls + b";\0" + b"MLBC" + struct.pack("<I", calls) + pattern[:calls]
        records[i] = struct.pack("<i", len(r) - 4 + len(fields)) + r[4:] + fields
        added += len(fields) - 17
    mergecases.write_raw_bam(os.path.join(d, "kinetics.bam"), text + "@RG\tID:movie1\tSM:sample\n", refs, records)
    print(json.dumps({"prepared": d, "records": len(records), "record_bytes": base + added + 17 * len(records), "kinetics_and_modification_bytes": added,
                      "share": round(added / (base + added + 17 * len(records)), 4), "file_bytes": os.path.getsize(os.path.join(d, "kinetics.bam"))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=16)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--out", required=True)
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--mode", choices=("off", "drop", "keep"), default=None)
    ap.add_argument("--root", default=HERE, help="the tree whose svision_amd is timed (default: this one)")
    ap.add_argument("--runs", type=int, default=1)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, os.path.join(root, "tools"))
    sys.path.insert(0, root)
    import torch
    from svision_amd import sort
    assert os.path.abspath(sort.__file__).startswith(root + os.sep), sort.__file__
    d = args.out
    os.makedirs(d, exist_ok=True)
    if args.prepare:
        prepare(args, d, os.path.join(d, "hifi.%d.%d.shuffled.bam" % (args.mb, args.coverage)))
    if args.mode is None:
        return
    src, out = os.path.join(d, "kinetics.bam"), os.path.join(d, "sorted.%s.%d.bam" % (args.mode, os.getpid()))
    kw = {"drop": dict(drop_tags=DROP), "keep": dict(keep_tags=KEEP), "off": {}}[args.mode]
    walls = []
    for i in range(args.runs + 1):                              # (the first run warms the allocator and the page cache)
        stats = {}
        t0 = time.perf_counter()
        sort.sort_bam(src, out, stats=stats, **kw)
        if i:
            walls.append(round(time.perf_counter() - t0, 4))
    seconds = stats["seconds"]
    digest = hashlib.sha256(open(out, "rb").read() + open(out + ".bai", "rb").read()).hexdigest()
    os.unlink(out)
    os.unlink(out + ".bai")
    print(json.dumps({"mode": args.mode, "root": root, "wall_seconds": walls, "records": stats["records"], "ranges": stats["ranges"],
                      "range_reads": stats.get("range_reads"), "spans": stats["spans"], "stream_bytes": stats["stream_bytes"],
                      "inflated_bytes": stats["inflated_bytes"], "compressed_bytes": stats["compressed_bytes"], "tags_mode": stats.get("tags_mode"),
                      "tags_records": stats.get("tags_records"), "tags_bytes": stats.get("tags_bytes"), "seconds": seconds,
                      "tags_share": round(seconds.get("tags", 0.0) / max(sum(seconds.values()), 1e-9), 6), "sha256": digest,
                      "max_memory_allocated": int(torch.cuda.max_memory_allocated())}))


if __name__ == "__main__":
    main()
