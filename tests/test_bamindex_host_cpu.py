"""The kernels of csrc/svx_bamindex.hip without a GPU: the kernel file compiled as plain C++ against tools/hostwave (a wave = 64 host
threads, __ballot a barrier exchange) into a stand-alone program with AddressSanitizer and UBSan, run on the index-build cases.
It checks what a device run cannot show: that no read goes behind the range's end -- the inflated bytes lie in a heap block of
exactly their size -- and, once more, svx_bam_find_starts's d_first / d_exit and svx_bam_walk_offsets against tests/baicases.walk."""
import bisect
import os
import shutil
import struct
import subprocess

import pytest

from tests import baicases, htslike

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_START = baicases.NO_START


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_path_factory.mktemp("hostwave") / "bamindex_host")
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unused-result",
                           "-x", "c++", "-I", os.path.join(ROOT, "tools", "hostwave"), "-pthread", "-o", out, os.path.join(ROOT, "tools", "hostwave", "bamindex_main.cpp")])
    return out


def write_case(path, w, b0=0, nb=None, entry=None, n_ref=None, stream=None, want=None):
    """Blocks [b0, b0 + nb) of a walked file as one range (tools/hostwave/bamindex_main.cpp reads the layout); ``want``: (d_first, d_exit)
    where the walk does not give them."""
    nb = len(w.coff) - b0 if nb is None else nb
    base = w.dst[b0]
    dst = [d - base for d in w.dst[b0:b0 + nb + 1]]
    raw = (stream or w.stream)[base:w.dst[b0 + nb]]
    entry = (w.header_end if entry is None else entry) - base
    lengths = [l for _n, l in w.references][:n_ref]
    if want is None:
        first = [NO_START] * nb
        for o in reversed([o - base for o in w.offsets if entry <= o - base < dst[-1]]):
            first[bisect.bisect_right(dst[:-1], o) - 1] = o
        ends = [o - base for o in w.offsets[1:]] + [len(w.stream) - base]
        ex = next((o - base for o, e in zip(w.offsets, ends) if o - base >= entry and e > dst[-1]), dst[-1])
        want = (first, [ex, 0])
    with open(path, "wb") as f:
        f.write(struct.pack("<4Q", nb, entry, len(lengths), len(raw)) + struct.pack("<%dQ" % (nb + 1), *dst))
        f.write(struct.pack("<%di" % ((len(lengths) + 1) // 2 * 2), *(lengths + [0] * (len(lengths) & 1))))
        f.write(raw + bytes(-len(raw) % 8))
        f.write(struct.pack("<%dQ" % nb, *want[0]) + struct.pack("<2Q", *want[1]))
    return path


def test_kernels_on_the_host_under_sanitizers(program, tmp_path):
    cases = []
    for name, recs, policy in (("flushed", baicases.short_records(n=120), "htslib"), ("straddling", baicases.short_records(seed=4, n=120), "stream"),
                               ("cg", baicases.short_records(seed=6, n=40, cg=True), "htslib")):
        path = str(tmp_path / (name + ".bam"))
        htslike.write_bam(path, baicases.REFS, recs, level=1, policy=policy, index=False)
        w = baicases.walk(path)
        cases.append(write_case(str(tmp_path / (name + ".case")), w))
        if name == "straddling":
            assert all(f % baicases.BLOCK for f in w.first[1:-1])
            cases.append(write_case(str(tmp_path / "every_guess_wrong.case"), w, n_ref=0))           # an empty dictionary: no candidate anywhere
            cases.append(write_case(str(tmp_path / "mid_range.case"), w, b0=2, nb=4, entry=w.first[2]))      # cut by the range's end
            s = bytearray(w.stream)
            s[w.offsets[50]:w.offsets[50] + 4] = struct.pack("<i", 7)
            cases.append(write_case(str(tmp_path / "block_size_7.case"), w, stream=bytes(s), want=([0] * len(w.coff), [w.offsets[50], 1])))
    wd, at = baicases.write_decoy(str(tmp_path / "decoy.bam"))
    assert at % baicases.BLOCK == 0 and wd.first[at // baicases.BLOCK] not in (at, NO_START)
    cases.append(write_case(str(tmp_path / "decoy.case"), wd))
    r = subprocess.run([program] + cases, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stdout.count(": ok") >= len(cases), r.stdout[-3000:] + r.stderr[-3000:]
