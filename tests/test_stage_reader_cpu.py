"""The staging reader of the device-side ingestion (csrc/svx_stage_core.hpp: a pool of pread threads that runs ahead through a ring
of slots with head-room, the BGZF block index per slot, the head of a cut block carried to the next slot) without a GPU:
tools/hostwave/stage_main.cpp drives it with a memcpy for the upload -- done as LATE as a copy on a stream may be -- into heap
buffers of exactly each range's size, once under AddressSanitizer + UBSan and once under ThreadSanitizer.  Nothing is loaded into
Python.  The assembled bytes must be the file's (the program compares them), the tables those of a serial scan of the file
(kernels.bgzf_block_table here), for every ring shape; every error path returns its code with all threads joined."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = 65536
SANITIZERS = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"], "tsan": ["-fsanitize=thread"]}
REPORTS = ("Sanitizer", "runtime error", "FAILED")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    d = tmp_path_factory.mktemp("hostwave")
    out = {}
    for name, flags in SANITIZERS.items():
        out[name] = str(d / ("stage_host_" + name))
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-g"] + flags + ["-o", out[name], os.path.join(ROOT, "tools", "hostwave", "stage_main.cpp"), "-lpthread"])
    return out


def _member(payload, level):
    """A BGZF block of ``payload``; level 0: ONE stored DEFLATE block (zlib would cut it into several)."""
    if level == 0:
        cdata = b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xFFFF) + payload
    else:
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        cdata = co.compress(payload) + co.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25) + cdata
            + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, bytes, block offsets + the end of the last block)."""
    d = tmp_path_factory.mktemp("stage_files")
    paths = {n: os.path.join(helpers.GOLDEN, n) for n in sorted(os.listdir(helpers.GOLDEN)) if n.endswith(".bam")}
    from svision_amd import synth
    table, _g, _ = synth.simulate(synth.SimConfig(contigs=[("c1", 400_000)], coverage=20, seed=4), with_genome=False)
    seg = bam.encode_reference_segment(table, seq="random", seed=1)
    paths["hifi"] = str(d / "hifi.bam")
    bam.write_bam_segments(paths["hifi"], table.references, table.lengths, [seg])
    paths["empties"] = str(d / "empties.bgzf")                                # 28-byte blocks: thousands per slot
    with open(paths["empties"], "wb") as f:
        f.write(_member(b"", 6) * 12_000)
    rng = np.random.default_rng(3)
    paths["stored"] = str(d / "stored.bgzf")                                  # stored blocks of the maximal 65,536 bytes
    with open(paths["stored"], "wb") as f:
        for _ in range(9):
            f.write(_member(bytes(rng.integers(0, 256, 65505, dtype=np.uint8)), 0))
    out = {}
    for name, path in paths.items():
        raw = np.fromfile(path, np.uint8)
        src_off, src_len, _isize, blk = kernels.bgzf_block_table(raw)
        ends = np.append(blk, src_off[-1] + src_len[-1] + 8).astype(np.int64)
        assert int(ends[-1]) == raw.size and (name != "stored" or set(np.diff(ends).tolist()) == {65536}) and (name != "empties" or set(np.diff(ends).tolist()) == {28})
        out[name] = (path, raw, ends)
    return out


def _run(program, path, out, ranges, configs, mode="run", threads=4):
    r = subprocess.run([program, path, out, str(threads), ",".join("%d-%d" % ab for ab in ranges), ",".join("%dx%d" % c for c in configs), mode],
                       capture_output=True, text=True, timeout=120)
    text = r.stdout + r.stderr
    assert not any(w in text for w in REPORTS), text[-4000:]
    assert r.stdout.count("closed: workers 0") == len(configs), text[-4000:]     # every ring was closed with every worker joined
    return r.returncode, r.stdout


def _codes(stdout):
    return [int(v) for v in re.findall(r"^range \d+: rc (-?\d+)", stdout, flags=re.M)]


def _tables(out, r):
    with open("%s.%d" % (out, r), "rb") as f:
        n, used = struct.unpack("<QQ", f.read(16))
        src_off, coff = np.frombuffer(f.read(8 * n), np.uint64), np.frombuffer(f.read(8 * n), np.uint64)
        src_len, isize = np.frombuffer(f.read(4 * n), np.uint32), np.frombuffer(f.read(4 * n), np.uint32)
    return used, src_off, src_len, isize, coff


def _check_tables(out, raw, ranges):
    """The tables the program wrote == a serial scan of the file's bytes [c0, c1), offsets counted from c0."""
    for r, (c0, c1) in enumerate(ranges):
        used, src_off, src_len, isize, coff = _tables(out, r)
        e_off, e_len, e_isize, e_blk = kernels.bgzf_block_table(raw[c0:c1])
        assert e_off.size > 0 and used == int(e_off[-1]) + int(e_len[-1]) + 8, (r, used)
        assert np.array_equal(src_off, e_off) and np.array_equal(src_len, e_len) and np.array_equal(isize, e_isize), r
        assert np.array_equal(coff, np.asarray(e_blk, np.uint64) + np.uint64(c0)), r


def _carry_sizes(ends, c0=0):
    """Slot sizes at which a block ends exactly at the first slot's end (nothing carried), one byte before it (one byte
    carried) and one byte behind it (the whole block but its last byte: 65,535 bytes of a full block)."""
    e = int(next(v for v in ends if v - c0 >= HEAD + 1)) - c0
    return [HEAD + e, HEAD + e + 1, HEAD + e - 1]


@pytest.mark.parametrize("san", sorted(SANITIZERS))
def test_bytes_and_tables_for_every_ring_shape(programs, files, tmp_path, san):
    for name, (path, raw, ends) in files.items():
        sizes = [128 << 10, 256 << 10] + _carry_sizes(ends)
        configs = [(s, n) for s in sizes for n in (2, 8)]
        ranges = [(0, raw.size)]                                                  # (ends at the end of the file)
        out = str(tmp_path / (name + ".tables"))
        rc, stdout = _run(programs[san], path, out, ranges, configs)
        assert rc == 0 and _codes(stdout) == [0] * len(configs), stdout[-2000:]
        _check_tables(out, raw, ranges)
    # the carry of the full blocks: slot payload = k blocks - 1 byte -> 65,535 bytes go to the next slot's head-room
    assert _carry_sizes(files["stored"][2])[2] == HEAD + 2 * 65536 - 1


@pytest.mark.parametrize("san", sorted(SANITIZERS))
def test_range_shapes(programs, files, tmp_path, san):
    path, raw, ends = files["hifi"]
    nb = ends.size - 1
    a, b = nb // 3, 2 * nb // 3
    # three ranges of one reader that overlap by one block each (a group's range takes its last unit's last block along), the last
    # one up to the end of the file; the read-ahead crosses from one into the next
    ranges = [(int(ends[0]), int(ends[a + 1])), (int(ends[a]), int(ends[b + 1])), (int(ends[b]), raw.size)]
    out = str(tmp_path / "overlap.tables")
    configs = [(128 << 10, 2), (128 << 10, 8), (256 << 10, 2), (256 << 10, 8)]
    rc, stdout = _run(programs[san], path, out, ranges, configs)
    assert rc == 0 and _codes(stdout) == [0] * (3 * len(configs)), stdout[-2000:]
    _check_tables(out, raw, ranges)
    # a range whose last slot holds only the head of a block: the first slot's payload ends at a block boundary, 100 bytes follow
    c0 = int(ends[2])
    cut = int(next(v for v in ends if v - c0 >= HEAD))
    ranges = [(c0, cut + 100)]
    out = str(tmp_path / "head_only.tables")
    rc, stdout = _run(programs[san], path, out, ranges, [(HEAD + cut - c0, 2), (HEAD + cut - c0, 8), (128 << 10, 2)])
    assert rc == 0 and _codes(stdout) == [0, 0, 0], stdout[-2000:]
    _check_tables(out, raw, ranges)
    assert _tables(out, 0)[0] == cut - c0


@pytest.mark.parametrize("san", sorted(SANITIZERS))
def test_error_paths_return_their_code_and_close(programs, files, tmp_path, san):
    path, raw, ends = files["hifi"]
    out = str(tmp_path / "unused")
    rings = [(128 << 10, 2), (128 << 10, 8)]
    # no BGZF magic at a range's start (the second range: the first is staged, the reads of the second are under way)
    rc, stdout = _run(programs[san], path, out, [(0, int(ends[40])), (int(ends[40]) + 5, raw.size)], rings)
    assert rc == 0 and _codes(stdout) == [0, -3] * 2 and "no BGZF block at file offset %d" % (int(ends[40]) + 5) in stdout, stdout[-2000:]
    # garbage in the third slot (payload [128 KB, 192 KB) of the file): the magic of the first block that starts there
    at = int(next(v for v in ends if v >= 2 * HEAD))
    assert at < 3 * HEAD
    bad = raw.copy()
    bad[at:at + 4] = 0
    bad_path = str(tmp_path / "garbage.bam")
    bad.tofile(bad_path)
    rc, stdout = _run(programs[san], bad_path, out, [(0, raw.size)], rings)
    assert rc == 0 and _codes(stdout) == [-4] * 2 and "no BGZF block at file offset %d" % at in stdout, stdout[-2000:]
    # a range that runs past the end of the file
    rc, stdout = _run(programs[san], path, out, [(0, raw.size + 100_000)], rings)
    assert rc == 0 and _codes(stdout) == [-2] * 2 and "short read" in stdout, stdout[-2000:]
    # the reader stopped in the middle of a range, with reads outstanding, and closed
    rc, stdout = _run(programs[san], path, out, [(0, raw.size)], rings, mode="stop3")
    assert rc == 0 and _codes(stdout) == [-6] * 2, stdout[-2000:]
    # closed right after the open; closed after the first range with the second one's reads outstanding
    rc, stdout = _run(programs[san], path, out, [(0, raw.size)], rings, mode="early")
    assert rc == 0 and _codes(stdout) == [], stdout[-2000:]
    rc, stdout = _run(programs[san], path, out, [(0, int(ends[40])), (int(ends[40]), raw.size)], rings, mode="abandon")
    assert rc == 0 and _codes(stdout) == [0] * 2, stdout[-2000:]
    # a ring the reader refuses: one slot, or slots that cannot hold a whole block behind the head-room
    r = subprocess.run([programs[san], path, out, "4", "0-%d" % raw.size, "131071x2", "run"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "open: rc -1" in r.stdout and not any(w in r.stdout + r.stderr for w in REPORTS)
