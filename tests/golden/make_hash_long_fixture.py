#!/usr/bin/env python3
"""Generates tests/golden/hash_long.expected.json.gz by calling the REFERENCE's hashplot_unmapped
(src/segmentplot/run_hash_lineplot.py:52 of the reference tree; pure Python, imported unmodified) on every case of
tests/hashcases_long.py: pieces of 2,049 to 65,537 bases on reference windows of up to 70,000 bases.

    python tests/golden/make_hash_long_fixture.py <root of the reference tree>

The fixture keeps per case its name, k, window, a CRC of the two sequences (the tests regenerate them from the name and
compare) and the reference's final segments -- no bases."""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True
from tests import hashcases, hashcases_long  # noqa: E402


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from src.segmentplot.run_hash_lineplot import hashplot_unmapped      # the reference's
    out = []
    for c in hashcases_long.all_cases():
        _m, segs = hashplot_unmapped(c.ref, c.seq, c.k, c.window)
        segs = [[s.xStart(), s.xEnd(), s.yStart(), s.yEnd(), bool(s.forward())] for s in segs]
        out.append({"name": c.name, "k": c.k, "window": c.window, "crc": hashcases.digest(c), "segs": segs})
        print(" ", c.name, len(c.seq), len(c.ref), "segments", len(segs))
    path = os.path.join(HERE, "hash_long.expected.json.gz")
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as f:   # mtime 0: regenerates byte for byte
        f.write(json.dumps({"cases": out}).encode())
    print("cases", len(out), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
