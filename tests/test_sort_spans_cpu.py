"""The plan of a sort in spans (svision_amd/sort.py: plan_spans, span_ranges, parse_memory) and the copy routine of the scatter kernel
(svision_amd/csrc/svx_recsort_core.hpp) without a GPU.

The plan is checked by its properties on crafted record lengths and budgets, and by a NumPy model of the whole placement: records
scattered range by range and span by span into span buffers whose kept parts, end to end, must be tests/sortcases.gather_segments'
stream.  The copy routine runs in a stand-alone program (tools/hostwave/scatter_main.cpp) under AddressSanitizer and UBSan, source and
destination in heap blocks of exactly their sizes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from svision_amd import sort
from tests import sortcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = sort.BLOCK


def _length_cases():
    scaled = sortcases.segment_lengths() * 700                  # 63 x 700 .. 70,000 x 700: several records above 0xFF00, the empty runs stay
    assert (scaled > BLOCK).sum() >= 3 and scaled[0] == 0 and scaled[-1] == 0
    return {"scaled": scaled, "ones": np.ones(3 * BLOCK + 17, np.int64), "one_long": np.asarray([300_000], np.int64), "none": np.zeros(0, np.int64),
            "all_empty": np.zeros(9, np.int64)}


def _offsets(lens):
    off = np.zeros(lens.size + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


def _budgets(total):
    return [1, BLOCK, BLOCK * 5 // 2, max(total, 1), total + 1]


@pytest.mark.parametrize("name", ["scaled", "ones", "one_long", "none", "all_empty"])
def test_plan_spans_properties(name):
    lens = _length_cases()[name]
    off = _offsets(lens)
    total, n = int(off[-1]), lens.size
    longest = int(lens.max()) if n else 0
    for budget in _budgets(total):
        plan = sort.plan_spans(off, budget)
        span_bytes = max(budget // BLOCK, 1) * BLOCK
        if total == 0:
            assert plan == []
            continue
        if budget >= total:
            assert len(plan) == 1
            span_bytes = total
        # the spans tile [0, total); all but the last are the same whole number of blocks
        assert plan[0].lo == 0 and plan[-1].hi == total
        assert all(a.hi == b.lo for a, b in zip(plan, plan[1:]))
        assert all(s.hi - s.lo == span_bytes for s in plan[:-1]) and 0 < plan[-1].hi - plan[-1].lo <= span_bytes
        lo, hi = np.asarray([s.lo for s in plan]), np.asarray([s.hi for s in plan])
        r_lo, r_hi = np.asarray([s.r_lo for s in plan]), np.asarray([s.r_hi for s in plan])
        assert (0 <= r_lo).all() and (r_lo < r_hi).all() and (r_hi <= n).all()
        for s in plan:
            assert s.base == off[s.r_lo] <= s.lo and off[s.r_hi] >= s.hi             # the buffer holds every byte of the span
            assert s.size == off[s.r_hi] - s.base + 4 <= (s.hi - s.lo) + 2 * longest + 4
        # a record with bytes lies in [r_lo, r_hi) of exactly the spans its bytes touch (spans x records, vectorised); one without
        # bytes touches none -- it may be listed where it lies strictly inside a span, never at an edge or outside
        a, b = off[:-1][None, :], off[1:][None, :]
        listed = (r_lo[:, None] <= np.arange(n)[None, :]) & (np.arange(n)[None, :] < r_hi[:, None])
        touches = (a < hi[:, None]) & (b > lo[:, None]) & (b > a)
        full = np.broadcast_to(b > a, listed.shape)
        assert np.array_equal(listed & full, touches)
        inside = (a > lo[:, None]) & (a < hi[:, None])
        assert not (listed & ~full & ~inside).any()


def _place_in_spans(data, off_in, order, range_records, budget):
    """The NumPy model of the spanned output: -> (the stream, reads of a range over all spans)."""
    n = order.size
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    lens = np.diff(off_in)
    off_out = _offsets(lens[order])
    rec_base = _offsets(np.asarray(range_records, np.int64))
    out, reads = [], 0
    for s in sort.plan_spans(off_out, budget):
        buf = np.full(s.size, 0xA5, np.uint8)
        for k in sort.span_ranges(rank, range_records, s.r_lo, s.r_hi):
            reads += 1
            for i in range(int(rec_base[k]), int(rec_base[k + 1])):        # the scatter kernel's launch over the range's records
                r = int(rank[i])
                if s.r_lo <= r < s.r_hi:
                    at = int(off_out[r]) - s.base
                    buf[at:at + int(lens[i])] = data[int(off_in[i]):int(off_in[i + 1])]
        out.append(buf[s.lo - s.base:s.hi - s.base])
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), reads


def test_placement_model_gives_the_gathered_stream():
    rng = np.random.default_rng(5)
    lens = sortcases.segment_lengths() * 3                      # 210,000 bytes in the long record: it spans several blocks
    off_in = _offsets(lens)
    data = rng.integers(0, 256, int(off_in[-1]), dtype=np.uint8)
    n = lens.size
    range_records = [7, 0, 20, 1, n - 28]
    for order in (rng.permutation(n), np.arange(n)):
        want, _off = sortcases.gather_segments(data, off_in, order)
        for budget in _budgets(int(off_in[-1])) + [3 * BLOCK]:
            got, _reads = _place_in_spans(data, off_in, order, range_records, budget)
            assert np.array_equal(got, want), budget


def test_span_ranges_against_a_loop():
    rng = np.random.default_rng(6)
    n = 500
    range_records = [0, 120, 1, 0, 200, 179, 0]
    rec_base = _offsets(np.asarray(range_records, np.int64))
    owner = np.repeat(np.arange(len(range_records)), range_records)
    for rank in (rng.permutation(n), np.arange(n)):
        for r_lo, r_hi in ((0, 0), (0, 1), (0, n), (120, 121), (119, 122), (250, 400), (n - 1, n)):
            brute = sorted({int(owner[i]) for i in range(n) if r_lo <= rank[i] < r_hi})
            got = sort.span_ranges(rank, range_records, r_lo, r_hi)
            assert got.tolist() == brute and all(range_records[k] for k in got)
    assert rec_base[-1] == n
    # a sorted input: every span reads the ranges it overlaps, in all at most ranges + spans
    lens = rng.integers(100, 5000, n)
    off = _offsets(lens)
    plan = sort.plan_spans(off, 3 * BLOCK)
    reads = sum(sort.span_ranges(np.arange(n), range_records, s.r_lo, s.r_hi).size for s in plan)
    assert len(plan) >= 4 and reads <= len(range_records) + len(plan)
    # a shuffled one (this seed): the three ranges of more than 100 records are read for every whole span
    rank = rng.permutation(n)
    assert all(set(sort.span_ranges(rank, range_records, s.r_lo, s.r_hi).tolist()) >= {1, 4, 5} for s in plan[:-1])


def test_parse_memory():
    assert [sort.parse_memory(t) for t in ("1", "131072", "128K", "128k", "64M", "8G", "2GB", " 5 ")] == [1, 131072, 131072, 131072, 64 << 20, 8 << 30, 2 << 30, 5]
    for bad in ("", "nonsense", "K", "-1", "0", "1.5G", "12T"):
        with pytest.raises(ValueError):
            sort.parse_memory(bad)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_path_factory.mktemp("hostwave") / "scatter_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", out, os.path.join(ROOT, "tools", "hostwave", "scatter_main.cpp")])
    return out


def test_copy_routine_on_the_host_under_sanitizers(program):
    """All four source skews x four destination alignments with every rank in the window and with a window in the middle, and two
    wrong lengths (status 1, that record's place untouched): the program compares the bytes and the 0xA5 sentinels itself, the
    sanitizers see every access outside the exact heap blocks."""
    lens = sortcases.segment_lengths()
    r = subprocess.run([program] + [str(int(v)) for v in lens], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stdout.count(": ok") == 4 * 4 * 2 + 2, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("status 1") == 2 and "0 failures" in r.stdout
