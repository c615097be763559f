"""bgzf_lz_table_kernel (csrc/svx_lz_table.hip: a block's LZ77 copies by pointer doubling in a table of u16 entries) without a
GPU: tools/hostwave/lz_table_main.cpp runs the kernel's own phase code (csrc/svx_lz_table_core.hpp) as loops over T threads, in
three orders of the racing reads and writes, under AddressSanitizer and UBSan -- table, sequence stream and output in heap
blocks of exactly their size -- and compares with zlib.  Inputs: every member of tests/inflate_cases.py, the golden BAMs, a
400 kb synthetic HiFi BAM and crafted blocks; the crafted SEQUENCE streams (a distance past the block's start, sums beyond
ISIZE: nothing zlib would write) are built into the program and always run."""
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from svision_amd import kernels
from svision_amd.io import bam
from tests import helpers
from tests import inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_path_factory.mktemp("hostwave") / "lz_table_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", out, os.path.join(ROOT, "tools", "hostwave", "lz_table_main.cpp"), "-lz"])
    return out


def _block(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    cdata = co.compress(payload) + co.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25) + cdata
            + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


def _summary(stdout, path):
    line = next(l for l in stdout.splitlines() if l.startswith(path + ": ok"))
    g = re.search(r"blocks (\d+) \(\+ (\d+) malformed skipped, (\d+) above 0xFF00 handed over\).* max (\d+),", line)
    return tuple(int(v) for v in g.groups())


def _expected(path):
    """-> (blocks the table takes, blocks zlib refuses or whose ISIZE is wrong, blocks above 0xFF00 bytes), by zlib."""
    raw = np.fromfile(path, np.uint8)
    src_off, src_len, isize, _blk = kernels.bgzf_block_table(raw)
    ok = skipped = handed = 0
    for o, n, z in zip(src_off.tolist(), src_len.tolist(), isize.tolist()):
        d = zlib.decompressobj(-15)
        try:
            good = len(d.decompress(raw[o:o + n].tobytes())) == z and d.eof
        except zlib.error:
            good = False
        if not good:
            skipped += 1
        elif z > 0xFF00:
            handed += 1
        else:
            ok += 1
    return ok, skipped, handed


def test_table_phases_on_the_host_under_sanitizers(program, tmp_path):
    files = {}
    # the catalogue of streams zlib never writes, its malformed members (skipped where zlib refuses them) and their neighbours
    members = [b for c in ic.build() for b, _d in c.members]
    cat = str(tmp_path / "catalogue.bgzf")
    with open(cat, "wb") as f:
        f.write(b"".join(members) + b"".join(b for _n, b in ic.malformed()) + b"".join(b for b, _d in ic.good_blocks()))
    files[cat] = None
    for n in ("collect_small.bam", "ont_small.bam", "hash_collect.bam"):
        files[os.path.join(helpers.GOLDEN, n)] = None
    from svision_amd import synth
    table, _g, _ = synth.simulate(synth.SimConfig(contigs=[("c1", 400_000)], coverage=20, seed=4), with_genome=False)
    seg = bam.encode_reference_segment(table, seq="random", seed=1)
    hifi = str(tmp_path / "hifi.bam")
    bam.write_bam_segments(hifi, table.references, table.lengths, [seg])
    files[hifi] = None
    # crafted blocks: the deepest chain (one value, distance 1, exactly 0xFF00 bytes), one byte more (refused: handed over), an empty
    # block, stored-only blocks, a match that reaches the block's first byte
    rng = np.random.default_rng(2)
    noise = bytes(rng.integers(0, 256, 40000, dtype=np.uint8))
    payloads = [(bytes(0xFF00), 9), (b"q" * 0xFF01, 9), (b"", 6), (noise, 0), (b"", 0), (b"abc" * 700, 9), (b"z" + noise[:300] + b"z" * 2000, 6)]
    crafted = str(tmp_path / "crafted.bgzf")
    with open(crafted, "wb") as f:
        f.write(b"".join(_block(p, level) for p, level in payloads))
    files[crafted] = None
    r = subprocess.run([program] + list(files), capture_output=True, text=True, timeout=900)
    tail = r.stdout[-4000:] + r.stderr[-4000:]
    assert r.returncode == 0 and "FAILED" not in r.stdout and "crafted: ok" in r.stdout, tail
    assert r.stdout.count(": ok") == len(files) + 1, tail
    for path in files:                                                    # every block of every file was run, or is accounted for
        blocks, skipped, handed, max_rounds = _summary(r.stdout, path)
        assert max_rounds <= 17, (path, max_rounds)
        assert (blocks, skipped, handed) == _expected(path) and blocks > 0, (path, blocks, skipped, handed)
        if path == cat:
            assert skipped == len(ic.malformed()) and handed >= 1             # (the catalogue holds blocks above 0xFF00 bytes)
        elif path == crafted:
            assert (skipped, handed) == (0, 1)
        else:
            assert (skipped, handed) == (0, 0)
    # the crafted sequence streams: the deepest chain resolves within the cap, the defects are flagged with the lane kernel's codes
    for name, status in (("run_distance1_0xFF00", 0), ("isize_0xFF01_refused", 10), ("empty", 0), ("stored_only", 0), ("match_to_first_byte", 0),
                         ("distance_past_the_start", 8), ("distance_past_the_start_second_batch", 8), ("output_overrun", 5), ("literal_overrun", 5),
                         ("short_stream", 7)):
        g = re.search(r"crafted %s: status (\d+), rounds (\d+)" % name, r.stdout)
        assert g and int(g.group(1)) == status and int(g.group(2)) <= 17, (name, g and g.groups())
