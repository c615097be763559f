"""GPU tests of the sparse first layer and the active-pixel lists on the crafted images of tests/conv1cases.py (-m gpu).

svx_encode_conv1_live and svx_alexnet_active_sets_live are called through the C ABI with the test's own buffers: what a launch must write
goes in as NaN, what it must leave alone as a finite sentinel that has to be there bit for bit afterwards.  Every list, count and row-mask
buffer is followed by a guard of sentinels one image long.

The first layer's pooled activations are compared with an fp64 convolution of the oracle's 0 / 255 image under a bound DERIVED from the
kernel's arithmetic (tests/conv1cases.conv1_ref64), its LRN with the fp64 LRN of the kernel's own pooled values at the project's tolerance
for that code (rtol 1e-5, atol 1e-6).  The touched masks, the background vector, the rows in front of a live count and everything about the
pixel lists are exact.

Bits 27 .. 31 of a touched word are outside what include/svx.h defines: every touched set here leaves them clear.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from svision_amd import _lib, kernels
from tests import conv1cases as k1
from tests.test_gpu_cnn_tiles import SENTINEL            # finite, negative (no ReLU output), exactly representable

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ISENT = -77777                       # the sentinel of the int32 buffers: no pixel id, no count, no row mask (bit 31 is set)
NAN = float("nan")
HW = (729, 169, 169, 169)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _live(live):
    return None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the first layer ----
def _encode(rec, w1, base, lrn, radius=2, alpha=2e-5, beta=0.75, k=1.0, live=None, fill=NAN, n=None):
    """svx_encode_conv1_live into buffers filled with ``fill`` / ISENT: (return code, d_y [rows, 12, 27, 27, 8], d_touched [rows, 27])."""
    rows = rec.shape[0]
    y = torch.full((rows, 12, 27, 27, 8), fill, dtype=torch.float32, device=DEV)
    t = torch.full((rows, 27), ISENT, dtype=torch.int32, device=DEV)
    lv = _live(live)
    rc = _lib.load().svx_encode_conv1_live(rec.data_ptr(), rows if n is None else n, w1.data_ptr(), base.data_ptr(), y.data_ptr(), lrn, radius, alpha,
                                           beta, k, t.data_ptr(), None if lv is None else lv.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, y, t


@functools.lru_cache(maxsize=None)
def _table():
    """The whole case table: (oracle masks bool [n, 227, 227, 3], touched bool [n, 27, 27], records on the device)."""
    masks = k1.oracle_masks(None)
    return masks, k1.touched_pixels(masks), _dev(k1.records())


def _ref64(masks, w1, base, chunk=128):
    """(pooled, bound) of conv1cases.conv1_ref64 as float64 [n, 96, 27, 27] on the device: torch's convolution in double, in chunks."""
    w = torch.from_numpy(w1).to(DEV).double().permute(3, 2, 0, 1).contiguous()
    both = torch.cat([w, w.abs()])
    b = torch.from_numpy(base).to(DEV).double().view(1, -1, 1, 1)
    pooled, bound = [], []
    for i in range(0, masks.shape[0], chunk):
        m = _dev(masks[i:i + chunk].copy()).permute(0, 3, 1, 2).double()          # (a copy: the cached masks are read-only)
        o = 255.0 * F.conv2d(m, both, stride=4)
        pooled.append(F.max_pool2d((b + o[:, :k1.C1]).clamp_min(0), 3, 2))
        bound.append(k1.SEQ_TERMS * k1.UNIT * F.max_pool2d(b.abs() + o[:, k1.C1:], 3, 2))
    return torch.cat(pooled), torch.cat(bound)


@functools.lru_cache(maxsize=None)
def _problem(name):
    """A weight set on the device with the fp64 reference of the whole table, computed once and only read afterwards."""
    w1, base = k1.WEIGHTS[name]()
    masks = _table()[0]
    pooled, bound = _ref64(masks, w1, base)
    ids = k1.group_ids("c")                                   # the device convolution is the NumPy restatement
    p_np, b_np = k1.conv1_ref64(masks[ids], w1, base)
    assert np.allclose(pooled[ids].permute(0, 2, 3, 1).cpu().numpy(), p_np, rtol=0, atol=1e-9)
    assert np.allclose(bound[ids].permute(0, 2, 3, 1).cpu().numpy(), b_np, rtol=1e-9, atol=0)
    return _dev(w1), _dev(base), pooled, bound


def _check_touched_and_background(y, t, tag):
    """Exact: the touched words are the oracle's pooled receptive fields; every pooled pixel whose bit is clear holds, bit for bit, the
    vector of the empty image's pixel (0, 0), in every image; the empty images hold nothing else."""
    _masks, touched, _rec = _table()
    got = t.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero((got != k1.to_words(touched)).any(1))
    assert bad.size == 0, (tag, [k1.cases()[i].name for i in bad[:5]])
    yi = _bits(y)
    e = k1.empty_ids()
    bg = yi[e[0], :, 0, 0, :].reshape(1, 12, 1, 1, 8).expand_as(yi)
    free = ~_dev(touched).view(-1, 1, 27, 27, 1)
    same = torch.where(free, yi, bg) == bg
    assert bool(same.all()), (tag, [k1.cases()[i].name for i in torch.nonzero(~same.flatten(1).all(1)).flatten()[:5].tolist()])
    assert torch.equal(yi[e], bg[e]), tag
    return yi[e[0], :, 0, 0, :].reshape(96)


@pytest.mark.parametrize("name", sorted(k1.WEIGHTS))
def test_pooled_activations_stay_within_the_bound_of_the_fmaf_chain(name):
    """lrn = 0 on the whole table (1,401 images), into NaN: every element within SEQ_TERMS * 2^-24 * S of the fp64 value, S = |base| + 255 *
    sum |w| over the window's set taps, max-pooled.  Set B separates the two starts of a pooled pixel: relu(base) = 50 where a window is
    empty, 0 where none is.  Measured on an MI355X, largest error / bound: set A 0.0056, set B 0.0053.  The background vector is
    relu(base), bit for bit."""
    w1, base, want, bound = _problem(name)
    rc, y, t = _encode(_table()[2], w1, base, 0)
    assert rc == _lib.SVX_OK
    got = kernels.from_c8(y).double()
    err = (got - want).abs()
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max())
    print("set %s: largest error / bound %.4g (largest error %.4g)" % (name, ratio, float(err.nan_to_num(nan=float("inf")).max())))
    inside = err <= bound                                     # (NaN compares false: an unwritten element fails here)
    worst = torch.nonzero(~inside.flatten(1).all(1)).flatten()[:5].tolist()
    assert not worst, (name, ratio, [k1.cases()[i].name for i in worst])
    bg = _check_touched_and_background(y, t, name)
    assert torch.equal(bg, _bits(base.clamp_min(0)))


@pytest.mark.parametrize("name", sorted(k1.WEIGHTS))
def test_lrn_of_the_kernel_s_own_pooled_values_and_the_background_identity(name):
    """lrn = 1 with the network's parameters and every row of cnncases.POOL_PARAMS (radius 0, 1, 5, 96; the rsqrt and the powf form), on
    the whole table: the touched masks and the background identity hold for each parameter set, the wrapper returns the same bits, and on
    the mixed cases the values are the fp64 LRN of the kernel's own lrn = 0 output (deterministic: integer atomicMax on float bits)."""
    w1, base, _want, _bound = _problem(name)
    rec = _table()[2]
    rc, y0, _t = _encode(rec, w1, base, 0)
    assert rc == _lib.SVX_OK
    rc, again, _t = _encode(rec, w1, base, 0)
    assert rc == _lib.SVX_OK and torch.equal(_bits(again), _bits(y0))
    ids = k1.mixed_ids()
    pooled = kernels.from_c8(y0[ids]).permute(0, 2, 3, 1).double().cpu().numpy()
    backgrounds = set()
    for pname, radius, alpha, beta, k in k1.lrn_params():
        rc, y, t = _encode(rec, w1, base, 1, radius, alpha, beta, k)
        assert rc == _lib.SVX_OK, pname
        backgrounds.add(tuple(_check_touched_and_background(y, t, (name, pname)).tolist()))
        yw, tw = kernels.encode_conv1(rec, w1, base, lrn=True, radius=radius, alpha=alpha, beta=beta, k=k, touched=True)
        assert torch.equal(_bits(yw), _bits(y)) and torch.equal(tw, t), pname
        got = kernels.from_c8(y[ids]).permute(0, 2, 3, 1).cpu().numpy()
        want = k1.lrn64(pooled, radius, alpha, beta, k)
        assert np.allclose(got, want, rtol=1e-5, atol=1e-6), (name, pname, float(np.nanmax(np.abs(got - want))))
    assert len(backgrounds) == len(k1.lrn_params())           # the parameters reach the kernel: as many different background vectors


def test_rows_do_not_depend_on_the_batch_and_stop_at_live():
    """The mixed cases (about 40 images), lrn 0 and 1: rows in front of min(live, n) are bit-identical to the launch without a live
    count, rows behind keep the sentinel; live = 0 writes nothing, live = n + 5 everything.  A batch of one image gives that image's
    row of the large launch."""
    w1, base, _want, _bound = _problem("A")
    ids = k1.mixed_ids()
    rec = _table()[2][ids].contiguous()
    n = len(ids)
    for lrn in (0, 1):
        rc, whole, _t = _encode(_table()[2], w1, base, lrn)
        rc2, full, tfull = _encode(rec, w1, base, lrn)
        assert rc == rc2 == _lib.SVX_OK and torch.equal(_bits(full), _bits(whole[ids]))
        for live in k1.live_values(n):
            m = min(live, n)
            rc, y, t = _encode(rec, w1, base, lrn, live=live, fill=SENTINEL)
            assert rc == _lib.SVX_OK
            assert torch.equal(_bits(y[:m]), _bits(full[:m])) and torch.equal(t[:m], tfull[:m]), (lrn, live)
            assert torch.equal(y[m:], torch.full_like(y[m:], SENTINEL)) and torch.equal(t[m:], torch.full_like(t[m:], ISENT)), (lrn, live)
            yw, tw = kernels.encode_conv1(rec, w1, base, lrn=bool(lrn), touched=True, live=_live(live))
            assert torch.equal(_bits(yw[:m]), _bits(full[:m])) and torch.equal(tw[:m], tfull[:m]), (lrn, live)
        for i in (0, n // 2, n - 2):
            rc, one, tone = _encode(rec[i:i + 1].contiguous(), w1, base, lrn)
            assert rc == _lib.SVX_OK and torch.equal(_bits(one), _bits(full[i:i + 1])) and torch.equal(tone, tfull[i:i + 1]), (lrn, i)


def test_encode_refuses_misaligned_weights_and_accepts_no_images():
    """d_w1 or d_base 4 bytes off a 16-byte boundary: SVX_EINVAL, nothing written.  n = 0: SVX_OK, nothing written."""
    w1, base, _want, _bound = _problem("A")
    rec = _table()[2][k1.group_ids("c")].contiguous()

    def off_by_4(t):
        buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=DEV)
        out = buf[1:1 + t.numel()]
        out.copy_(t.reshape(-1))
        assert out.data_ptr() % 16 == 4
        return out

    for w, b in ((off_by_4(w1), base), (w1, off_by_4(base)), (off_by_4(w1), off_by_4(base))):
        for lrn in (0, 1):
            rc, y, t = _encode(rec, w, b, lrn, fill=SENTINEL)
            assert rc == _lib.SVX_EINVAL
            assert torch.equal(y, torch.full_like(y, SENTINEL)) and torch.equal(t, torch.full_like(t, ISENT))
            with pytest.raises(_lib.SvxError):
                kernels.encode_conv1(rec, w.view(w1.shape), b, lrn=bool(lrn))
    rc, y, t = _encode(rec, w1, base, 1, fill=SENTINEL, n=0)
    assert rc == _lib.SVX_OK
    assert torch.equal(y, torch.full_like(y, SENTINEL)) and torch.equal(t, torch.full_like(t, ISENT))
    assert _lib.load().svx_encode_conv1_live(None, 0, None, None, None, 1, 2, 2e-5, 0.75, 1.0, None, None, _stream()) == _lib.SVX_OK


# ---- the active sets ----
TOTALS0 = (1000, 2000, 3000, 4000, 5000)


def _check_active_sets(touched, live, tag):
    """Two launches of svx_alexnet_active_sets_live over touched bool [n, 27, 27] into sentinel-filled lists, counts and row masks (a
    guard of one image behind each) and running totals that already hold values; everything against conv1cases.expected_active_sets."""
    n = touched.shape[0]
    m = n if live is None else min(live, n)
    words = _dev(k1.to_words(touched).view(np.int32))
    lists = [torch.full(((n + 1) * hw,), ISENT, dtype=torch.int32, device=DEV) for hw in HW]
    counts = torch.full((4 + 4,), ISENT, dtype=torch.int32, device=DEV)
    rows2 = torch.full((n + 1, 27), ISENT, dtype=torch.int32, device=DEV)
    ws = torch.zeros(4 * n + 4, dtype=torch.int32, device=DEV)
    totals = torch.tensor(TOTALS0, dtype=torch.int64, device=DEV)
    lv = _live(live)
    assert ws.data_ptr() % 16 == 0
    for _launch in range(2):
        rc = _lib.load().svx_alexnet_active_sets_live(words.data_ptr(), n, lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(),
                                                      lists[3].data_ptr(), counts.data_ptr(), ws.data_ptr(), totals.data_ptr(), rows2.data_ptr(),
                                                      None if lv is None else lv.data_ptr(), _stream())
        assert rc == _lib.SVX_OK, tag
    torch.cuda.synchronize()
    want_lists, want_counts, want_rows, add = k1.expected_active_sets(touched, live)
    assert counts.cpu().tolist() == want_counts + [ISENT] * 4, (tag, counts.cpu().tolist(), want_counts)
    for li, (lst, hw) in enumerate(zip(lists, HW)):
        got = lst.cpu().numpy()
        assert np.array_equal(got[:m * hw], want_lists[li]), (tag, li)                       # active first, ascending, then the others
        assert np.array_equal(got[m * hw:], np.full((n + 1 - m) * hw, ISENT, np.int32)), (tag, li)
    got = rows2.cpu().numpy()
    assert np.array_equal(got[:m].view(np.uint32), want_rows) and np.array_equal(got[m:], np.full((n + 1 - m, 27), ISENT, np.int32)), tag
    assert totals.cpu().tolist() == [t0 + 2 * a for t0, a in zip(TOTALS0, add)], (tag, totals.cpu().tolist(), add)
    return want_counts, add


def _crafted_touched():
    return _table()[1][k1.mixed_ids()]


def test_active_sets_of_one_touched_pixel_at_every_position():
    """729 images with one touched pixel each, cut to 1, 255, 256, 257 and 729 images: more images than the workgroup of the lists
    kernel has threads for its prefix sums.  Each with live = 1, n - 1, n, n + 5 and without a live count."""
    single = k1.single_bit_touched()
    for n in k1.SINGLE_CUTS:
        for live in [None] + [v for v in k1.live_values(n) if v]:
            counts, add = _check_active_sets(single[:n], live, ("single", n, live))
            assert add[4] == n and 0 < counts[0] <= 25 * n


def test_active_sets_of_empty_full_and_crafted_images():
    for name, touched in (("empty and full", k1.empty_and_full_touched()), ("crafted", _crafted_touched())):
        n = touched.shape[0]
        for live in [None] + [v for v in k1.live_values(n) if v]:
            _check_active_sets(touched, live, (name, live))
    counts, _add = _check_active_sets(np.zeros((3, 27, 27), bool), None, "empty")
    assert counts == [0, 0, 0, 0]
    counts, add = _check_active_sets(np.ones((3, 27, 27), bool), None, "full")
    assert counts == add[:4] == [3 * hw for hw in HW]


def test_active_sets_totals_at_the_dense_threshold_and_one_pixel_below():
    """Three full images and a partial one: with conv2's list exactly SVX_CONV_DENSE_PCT percent full the totals advance by every pixel,
    one pixel below by the listed ones only."""
    at, total = k1.threshold_touched(0)
    below, total_below = k1.threshold_touched(1)
    every = at.shape[0] * 729
    counts, add = _check_active_sets(at, None, "at the threshold")
    assert counts[0] == total and add[0] == every
    counts, add = _check_active_sets(below, None, "below the threshold")
    assert counts[0] == total_below == total - 1 and add[0] == total - 1
    for live in (v for v in k1.live_values(at.shape[0]) if v):
        _check_active_sets(at, live, ("at", live))
        _check_active_sets(below, live, ("below", live))


def test_active_sets_without_a_live_image_zero_the_counts_and_count_the_launch():
    """live = 0 on n > 0 images (include/svx.h: d_counts and the pixel totals count the live images, the image total still adds n):
    d_counts = [0, 0, 0, 0], the lists and the row masks untouched, d_totals[4] advanced by n, the pixel totals not at all."""
    sets = [k1.single_bit_touched()[:n] for n in k1.SINGLE_CUTS] + [k1.empty_and_full_touched(), _crafted_touched(), k1.threshold_touched(0)[0]]
    for touched in sets:
        counts, add = _check_active_sets(touched, 0, ("live 0", touched.shape[0]))
        assert counts == [0, 0, 0, 0] and add == [0, 0, 0, 0, touched.shape[0]]
