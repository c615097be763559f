"""svx_record_invert and svx_record_scatter_segments (svision_amd/csrc/svx_recsort.hip) against NumPy (tests/sortcases.py): the inverse
permutation equals ``np.argsort(order)``; the scatter puts the records of a window of ranks where tests/sortcases.gather_segments puts
them -- every destination alignment, source offsets that are not dword aligned, empty and 70,000-byte segments --, leaves every other
byte at its sentinel, reports a record whose length does not fit without copying it, and gives the same bytes in a second launch."""
import numpy as np
import pytest
import torch

from svision_amd import kernels
from tests import sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = kernels.RECORD_SORT_TILE
GUARD = 0xA5
FRONT, BACK = 8, 16                                             # sentinel bytes in front of and behind the output stream's bytes
OFF = 1001                                                      # the stream offset of rank 0 (as if 1,001 bytes lay in front): out_base is odd


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1])
def test_invert(n):
    order = np.random.default_rng(n).permutation(n).astype(np.int32)
    rank = kernels.record_invert(torch.from_numpy(order).to(DEV)).cpu().numpy()
    assert np.array_equal(rank, np.argsort(order).astype(np.int32))


@pytest.fixture(scope="module")
def case():
    """The segments of tests/sortcases.segment_lengths in a source that starts 3 bytes into its array, a random order whose LAST five
    ranks are empty segments, and the NumPy gather of it: computed once, never changed."""
    rng = np.random.default_rng(17)
    lens = sortcases.segment_lengths()
    n = lens.size
    assert (lens[:5] == 0).all() and lens.max() == 70_000
    order = np.concatenate([5 + rng.permutation(n - 5), np.arange(5)]).astype(np.int64)
    rank = np.argsort(order)
    src_off = np.zeros(n + 1, np.int64)
    src_off[0] = 3
    src_off[1:] = 3 + np.cumsum(lens)
    assert len(set((src_off[:-1][lens > 0] % 4).tolist())) == 4
    src = np.zeros((int(src_off[n]) + 3) // 4 * 4, np.uint8)     # readable up to the next multiple of 4 behind its last byte, not further
    src[:] = rng.integers(0, 256, src.size, dtype=np.uint8)
    want, off_out = sortcases.gather_segments(src, src_off, order)
    assert len(set((FRONT + off_out[:-1][lens[order] > 0]) % 4)) == 4
    c = dict(n=n, lens=lens, order=order, rank=rank, src_off=src_off, src=src, want=want, off_out=off_out, total=int(off_out[n]))
    c["d_src"] = torch.from_numpy(src).to(DEV)
    c["d_src_off"] = torch.from_numpy(src_off).to(DEV)
    c["d_rank"] = torch.from_numpy(rank.astype(np.uint32).view(np.int32)).to(DEV)
    c["d_off_out"] = torch.from_numpy(off_out + OFF).to(DEV)
    return c


def _scatter(c, windows, parts=None, d_off_out=None, extra=0):
    """One launch per window of ranks and per part [a, b) of the input records into a sentinel-filled buffer -> (the buffer, status)."""
    d_buf = torch.full((FRONT + c["total"] + extra + BACK,), GUARD, dtype=torch.uint8, device=DEV)
    d_status = torch.zeros(1, dtype=torch.int32, device=DEV)
    for lo, hi in windows:
        for a, b in parts or [(0, c["n"])]:
            kernels.record_scatter_segments(c["d_src"], c["d_src_off"][a:b + 1], c["d_rank"][a:b], lo, hi,
                                            c["d_off_out"] if d_off_out is None else d_off_out, OFF - FRONT, d_buf, d_status)
    return d_buf.cpu().numpy(), int(d_status.item())


def _expected(c, windows):
    out = np.full(FRONT + c["total"] + BACK, GUARD, np.uint8)
    for lo, hi in windows:
        a, b = int(c["off_out"][lo]), int(c["off_out"][hi])
        out[FRONT + a:FRONT + b] = c["want"][a:b]
    return out


def test_windows(case):
    c, n = case, case["n"]
    big = int(case["rank"][int(np.argmax(case["lens"]))])
    windows = {"empty": (7, 7), "one_rank": (big, big + 1), "first_5": (0, 5), "last_5": (n - 5, n), "middle": (n // 3, 2 * n // 3), "all": (0, n)}
    for name, w in windows.items():
        got, status = _scatter(c, [w])
        assert status == 0 and np.array_equal(got, _expected(c, [w])), name
    assert (_scatter(c, [windows["last_5"]])[0] == GUARD).all()                      # five empty segments: nothing is written
    assert (_expected(c, [windows["one_rank"]]) != GUARD).sum() > 60_000


def test_disjoint_windows_and_ranges_give_the_gather(case):
    c, n = case, case["n"]
    full = _expected(c, [(0, n)])
    assert np.array_equal(full[FRONT:FRONT + c["total"]], c["want"])
    cuts = [(0, 5), (5, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    got, status = _scatter(c, cuts)
    assert status == 0 and np.array_equal(got, full)
    # the input records as three "ranges", a launch each
    got, status = _scatter(c, [(0, n)], parts=[(0, 20), (20, 45), (45, n)])
    assert status == 0 and np.array_equal(got, full)
    got, status = _scatter(c, cuts, parts=[(0, 20), (20, 45), (45, n)])
    assert status == 0 and np.array_equal(got, full)
    # svx_record_gather_segments from the same source
    d_out = torch.full((c["total"] + 4,), GUARD, dtype=torch.uint8, device=DEV)
    kernels.record_gather_segments(c["d_src"], c["d_src_off"], torch.from_numpy(c["order"].astype(np.uint32).view(np.int32)).to(DEV),
                                   torch.from_numpy(c["off_out"]).to(DEV), d_out)
    assert np.array_equal(d_out.cpu().numpy()[:c["total"]], full[FRONT:FRONT + c["total"]])


def test_a_wrong_length_is_reported_and_not_copied(case):
    c, n = case, case["n"]
    w = int(c["rank"][int(np.flatnonzero(c["lens"] == 65)[0])])                      # a record in the middle of the order, 65 bytes
    assert 0 < w < n - 6
    off_wrong = c["off_out"].copy()
    off_wrong[w + 1:] += 1                                      # rank w a byte longer in the output's offsets, every later rank a byte on
    got, status = _scatter(c, [(0, n)], d_off_out=torch.from_numpy(off_wrong + OFF).to(DEV), extra=1)
    want = np.full(FRONT + c["total"] + 1 + BACK, GUARD, np.uint8)
    for r in range(n):
        if r != w:
            a, b = int(c["off_out"][r]), int(c["off_out"][r + 1])
            want[FRONT + int(off_wrong[r]):FRONT + int(off_wrong[r]) + b - a] = c["want"][a:b]
    assert status == 1 and np.array_equal(got, want)
    assert (got[FRONT + int(off_wrong[w]):FRONT + int(off_wrong[w + 1])] == GUARD).all()


def test_a_second_launch_gives_the_same_bytes(case):
    n = case["n"]
    a, b = _scatter(case, [(0, n)]), _scatter(case, [(0, n)])
    assert a[1] == b[1] == 0 and np.array_equal(a[0], b[0])
    # and over a buffer that holds the bytes already: both launches into ONE buffer
    got, status = _scatter(case, [(0, n), (0, n)])
    assert status == 0 and np.array_equal(got, a[0])


def test_refusals(case):
    from svision_amd import _lib
    with pytest.raises(_lib.SvxError):
        _scatter(case, [(5, 4)])
    with pytest.raises(_lib.SvxError):
        _scatter(case, [(0, case["n"] + 1)])
