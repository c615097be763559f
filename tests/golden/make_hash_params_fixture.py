#!/usr/bin/env python3
"""Generates tests/golden/hash_params.expected.json.gz by calling the REFERENCE's hashplot_unmapped
(src/segmentplot/run_hash_lineplot.py:52 of the reference tree; pure Python, imported unmodified) on every case of
tests/hashcases.py: k from 2 to 14, windows of 2 to 120 bases, pieces of up to 2049 bases, reference windows of up to
20,000 bases, the alphabet ACGTNacgtnRYKMS.

    python tests/golden/make_hash_params_fixture.py <root of the reference tree>

The fixture keeps per case its name, k, window, a CRC of the two sequences (the tests regenerate them from the name and
compare) and the reference's final segments -- no bases.

Counts of the committed fixture: 143 cases; with a non-empty result, per group: a 43 of 72 (k7w30 7, k10w10 9, k10w120 7,
k12w30 6, k13w13 8, k13w50 6, of 12 each, 9 of which carry a planted copy), b 3 of 12, c 7 of 10, d 2 of 2, e 1 of 1,
f 1 of 1, g 8 of 42, k14 2 of 3.  The reference needs about 1.5 s for all of them."""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
from tests import hashcases  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from src.segmentplot.run_hash_lineplot import hashplot_unmapped      # the reference's
    out, groups = [], {}
    for c in hashcases.all_cases():
        _m, segs = hashplot_unmapped(c.ref, c.seq, c.k, c.window)
        segs = [[s.xStart(), s.xEnd(), s.yStart(), s.yEnd(), bool(s.forward())] for s in segs]
        out.append({"name": c.name, "k": c.k, "window": c.window, "crc": hashcases.digest(c), "segs": segs})
        g = c.name.split("/")[0] if not c.name.startswith("a/") else "a/" + hashcases.sweep_group(c)
        n, h = groups.get(g, (0, 0))
        groups[g] = (n + 1, h + bool(segs))
    path = os.path.join(HERE, "hash_params.expected.json.gz")
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as f:   # mtime 0: regenerates byte for byte
        f.write(json.dumps({"cases": out}).encode())
    print("cases", len(out), "bytes", os.path.getsize(path))
    for g, (n, h) in groups.items():
        print(" ", g, n, "with segments", h)


if __name__ == "__main__":
    main()
