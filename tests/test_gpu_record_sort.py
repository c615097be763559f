"""svx_record_sort and the gathers (svision_amd/csrc/svx_recsort.hip) against NumPy (tests/sortcases.py): the permutation equals
``np.argsort(key, kind="stable")`` exactly -- sizes around the wave and the tile, key patterns that single out a digit, a pass or
the tie order -- and two runs over a dirty workspace are byte-identical; the gathers equal fancy indexing and write nothing
outside their output."""
import numpy as np
import pytest
import torch

from svision_amd import _lib, kernels
from tests import sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = kernels.RECORD_SORT_TILE
GUARD = 0xA5


CASES = {c[0]: c[1:] for c in sortcases.key_cases(T)}


def device_order(tid, pos, n_ref, pos_bits):
    d = kernels.record_sort(torch.from_numpy(tid).to(DEV), torch.from_numpy(pos).to(DEV), n_ref, pos_bits)
    return d.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_order_equals_stable_argsort(name):
    tid, pos, n_ref, pos_bits = CASES[name]
    want = sortcases.order(tid, pos, n_ref).astype(np.uint32)
    got = device_order(tid, pos, n_ref, pos_bits)
    assert got.shape == want.shape
    assert np.array_equal(got, want), (name, int(np.flatnonzero(got != want)[0]))
    again = device_order(tid, pos, n_ref, pos_bits)             # the allocator hands the same, now dirty, workspace back
    assert got.tobytes() == again.tobytes()


def test_the_cases_cover_what_they_claim():
    c = CASES
    sizes = sorted(v[0].size for k, v in c.items() if k.startswith("random/n"))
    assert sizes == [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1, 300_001, 2_200_003]
    assert 256 * ((300_001 + T - 1) // T) > 4 * 1024 and (2_200_003 + T - 1) // T * 256 // 1024 > 256      # scan chunks; steps of its top level
    tid, pos, n_ref, _bits = c["all_equal"]
    assert tid.size > 3 * T and np.unique(sortcases.key(tid, pos, n_ref)).size == 1
    assert np.unique(sortcases.key(*c["alternating"][:3])).size == 2
    k = sortcases.key(*c["sorted"][:3])
    assert (k[1:] >= k[:-1]).all()
    k = sortcases.key(*c["reversed"][:3])
    assert (k[1:] <= k[:-1]).all()
    k = sortcases.key(*c["top_digit_only"][:3])
    assert np.unique(k & np.uint64((1 << 40) - 1)).size == 1 and np.unique(k >> np.uint64(40)).size > 8
    k = sortcases.key(*c["low_digit_only"][:3])
    assert np.unique(k >> np.uint64(8)).size == 1 and {0, 255} <= set((k & np.uint64(255)).tolist())
    tid, pos, _n_ref, _bits = c["max_pos_and_unmapped"]
    assert int(pos.max()) == (1 << 31) - 2 and (tid[:100] == -1).any() and (tid[-100:] == -1).any()


def test_refusals():
    lib = _lib.load()
    d = torch.zeros(8, dtype=torch.int32, device=DEV)
    ws = torch.zeros(int(lib.svx_record_sort_ws_bytes(8)), dtype=torch.uint8, device=DEV)
    sp = kernels._stream_ptr(torch.device(DEV))
    out = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    for pos_bits, ws_bytes in ((0, ws.numel()), (33, ws.numel()), (25, ws.numel() - 1)):
        assert lib.svx_record_sort(d.data_ptr(), d.data_ptr(), 8, 2, pos_bits, out.data_ptr(), ws.data_ptr(), ws_bytes, sp) == _lib.SVX_EINVAL
    assert lib.svx_record_gather(d.data_ptr(), d.data_ptr(), out.data_ptr(), 8, 3, sp) == _lib.SVX_EINVAL
    assert lib.svx_record_gather_segments(d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), out.data_ptr(), 8, 8, sp) == _lib.SVX_EINVAL
    torch.cuda.synchronize()
    assert out.tolist() == [-7] * 8


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
def test_fixed_width_gather(dtype):
    rng = np.random.default_rng(5)
    for n in (0, 1, 65, 3 * T + 1):
        src = rng.integers(0, 120, n).astype(dtype)
        rows = rng.permutation(n).astype(np.int32)
        got = kernels.record_gather(torch.from_numpy(src).to(DEV), torch.from_numpy(rows).to(DEV))
        assert got.dtype == torch.from_numpy(src).dtype and np.array_equal(got.cpu().numpy(), src[rows])


def segmented(lens, dtype, rows, front):
    """One segmented gather with guard bytes around the output, ``front`` elements in front of it -> checked against the oracle."""
    rng = np.random.default_rng(int(lens.sum()) + front)
    off = np.zeros(lens.size + 1, np.int64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    data = rng.integers(1, 100, total).astype(dtype)
    want_data, want_off = sortcases.gather_segments(data, off, rows)
    item = np.dtype(dtype).itemsize
    src = np.zeros(total + 4, dtype)                            # (readable up to the next multiple of 4 bytes behind its end)
    src[:total] = data
    d_src, d_off = torch.from_numpy(src).to(DEV), torch.from_numpy(off).to(DEV)
    d_rows = torch.from_numpy(rows.astype(np.int32)).to(DEV)
    d_off_out = kernels.record_gather_offsets(d_off, d_rows)
    assert np.array_equal(d_off_out.cpu().numpy(), want_off)
    back = 64
    guard = np.frombuffer(bytes([GUARD]) * item, dtype)[0]
    d_out = torch.full((front + total + back,), int(guard), dtype=d_src.dtype, device=DEV)
    kernels.record_gather_segments(d_src, d_off, d_rows, d_off_out, d_out[front:front + max(total, 1)])
    out = d_out.cpu().numpy()
    assert np.array_equal(out[front:front + total], want_data)
    assert (out[:front] == guard).all() and (out[front + total:] == guard).all()      # nothing outside [0, total)


@pytest.mark.parametrize("dtype", [np.int32, np.uint8, np.int16])
def test_segmented_gather(dtype):
    lens = sortcases.segment_lengths()
    n = lens.size
    rng = np.random.default_rng(9)
    item = np.dtype(dtype).itemsize
    for k in range(4 // item):                                  # every alignment of the output against a dword
        segmented(lens, dtype, rng.permutation(n), 16 + k)
    segmented(lens, dtype, np.arange(n), 16)                    # the identity: zero-length runs first and last stay there
    segmented(lens, dtype, np.arange(n)[::-1].copy(), 16)
    for one in (0, 1, 5, 70_000):                               # n = 1
        segmented(np.asarray([one], np.int64), dtype, np.zeros(1, np.int64), 16)
    segmented(np.zeros(9, np.int64), dtype, rng.permutation(9), 16)      # nothing but empty segments
