"""GPU tests of the CNN matrix kernels at every tile shape, loop tail and grid edge (-m gpu).

svx_conv2d_same, svx_fc_bias_act, svx_bias_relu_pool_lrn and svx_fc8_softmax against fp64 references of the same operation, at the
shapes of tests/cnncases.py: the restated planning rules there say, for the device the test runs on, which wave tile shape, loop tail and
work distribution a case takes, and the tests assert that on the host before they launch.  The tolerances are the project's own (conv
2e-4 and fc 2e-5 of the reference's largest magnitude, pool/LRN rtol 1e-5 / atol 1e-6).

Every buffer a kernel is meant to fill goes in pre-filled with NaN, so a tile no wave computes fails the comparison; where rows or pixels
must stay untouched the buffer holds a finite sentinel, which has to be there bit for bit afterwards.

On a whole MI355X (256 CUs, 1,024 SIMDs) the searches choose: dense shape 1 at 12 images (conv2, 5x5) and 33 images (conv3, 3x3), shape
0 at 11 and 32; list mode on 12 images with 8,193 / 8,192 listed pixels (conv2) and on 34 images with 5,441 / 5,440 (conv3).  Run with -s,
the tests print what they chose on the device at hand.

Dense tile shapes 2, 3 and 4 of svx_conv.hip are not tested because they cannot run: conv_pick_shape never picks them, for any size
(tests/cnncases.py has the argument, tests/test_cnncases_cpu.py scans it), and only an experiment build can force them.  A clean-up that
removes them loses no tested path.

One undefined shift is known and harmless on this hardware: bias_relu_pool_lrn_kernel evaluates rows[dy] >> (2 * ox + dx) with a
count of 32 or more when width > 32 and no row masks are given (the entry point refuses masks at that width).  rows is then all ones, the
hardware shift takes the count modulo 32, and the bit read is 1 either way; the "width 33" case below runs it against fp64.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import alexnet_ref
from svision_amd import _lib, kernels
from tests import cnncases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONV_TOL, FC_TOL = 2e-4, 2e-5
SENTINEL = -7777.25                  # finite, negative (no ReLU output), exactly representable


def _n_simd():
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count          # device_simds() of svx_conv.hip


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _int1(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


# ---- convolution ----
class _Conv:
    """One convolution problem on the device with its fp64 result (bias added, no ReLU), computed once and only read afterwards."""

    def __init__(self, seed, n, cin, cout, h, w, ksize, groups):
        rng = np.random.default_rng(seed)
        self.n, self.cin, self.cout, self.h, self.w, self.ksize, self.groups = n, cin, cout, h, w, ksize, groups
        cin_g = cin // groups
        self.x = _dev(rng.standard_normal((n, cin, h, w)).astype(np.float32))
        self.w_hwio = _dev((rng.standard_normal((ksize, ksize, cin_g, cout)) / np.sqrt(ksize * ksize * cin_g)).astype(np.float32))
        self.b = _dev(rng.standard_normal(cout).astype(np.float32))
        self.want = F.conv2d(self.x.double(), self.w_hwio.permute(3, 2, 0, 1).contiguous().double(), self.b.double(), 1, ksize // 2, 1, groups)
        self.xc, self.wp = kernels.to_c8(self.x), kernels.pack_conv_weights(self.w_hwio)

    def out(self, n, fill):
        return torch.full((n, self.cout // 8, self.h, self.w, 8), fill, dtype=torch.float32, device=DEV)

    def dense(self, n=None, bias=True, relu=False):
        n = self.n if n is None else n
        y = kernels.conv2d_same(self.xc[:n], self.wp, self.b if bias else None, groups=self.groups, relu=relu, out=self.out(n, float("nan")))
        return kernels.from_c8(y)

    def check_dense(self, n=None, variants=True):
        """bias, no bias and bias + ReLU, each into a NaN-filled buffer, against fp64."""
        n = self.n if n is None else n
        want = self.want[:n]
        tol = CONV_TOL * float(want.abs().max())
        errs = [float((self.dense(n).double() - want).abs().max())]
        if variants:
            errs.append(float((self.dense(n, bias=False).double() + self.b.double().view(1, -1, 1, 1) - want).abs().max()))
            errs.append(float((self.dense(n, relu=True).double() - want.clamp_min(0)).abs().max()))
        for e in errs:
            assert e < tol, (e, tol)                          # (NaN compares false: an unwritten element fails here)
        return max(errs) / tol

    def check_list(self, active, n=None, background=False, live=None):
        """List mode with bias + ReLU (the production call).  ``active``: ascending pixel ids within the covered images.  Computed pixels
        equal the fp64 convolution, the other pixels of the covered images the background bit for bit (or, without one, the sentinel),
        images behind ``live`` the sentinel."""
        n = self.n if n is None else n
        hw = self.h * self.w
        covered = n if live is None else min(live, n)
        mall = covered * hw
        active = np.asarray(active, np.int64)
        count = int(active.size)
        lst = np.concatenate([cc.pixel_list(active, mall), np.arange(mall, n * hw, dtype=np.int32)])      # (behind mall: never read)
        computed = np.zeros(n * hw, bool)
        if cc.list_is_followed(count, mall):
            computed[active] = True
        else:
            computed[:mall] = True
        copied = np.zeros(n * hw, bool)
        if background:
            copied[:mall] = ~computed[:mall]
        untouched = ~(computed | copied)
        bg = _dev(np.random.default_rng(count).standard_normal((self.cout, self.h, self.w)).astype(np.float32)) if background else None
        out = self.out(n, SENTINEL if untouched.any() else float("nan"))
        y = kernels.conv2d_same(self.xc[:n], self.wp, self.b, groups=self.groups, relu=True, pixels=_dev(lst), pixel_count=_int1(count), out=out,
                                background=kernels.to_c8(bg.unsqueeze(0))[0] if background else None, live=None if live is None else _int1(live))
        assert y.data_ptr() == out.data_ptr()
        got = kernels.from_c8(y)
        want = self.want[:n].clamp_min(0)
        comp = _dev(computed).view(n, 1, self.h, self.w)
        err = float(torch.where(comp, (got.double() - want).abs(), torch.zeros_like(want)).max())
        assert err < CONV_TOL * float(want.abs().max()), (count, err)
        if background:
            bgx = bg.unsqueeze(0).expand(n, -1, -1, -1)
            assert torch.equal(torch.where(_dev(copied).view(n, 1, self.h, self.w), got, bgx), bgx), count
        keep = torch.full_like(got, SENTINEL)
        assert torch.equal(torch.where(_dev(untouched).view(n, 1, self.h, self.w), got, keep), keep), count
        return int(computed.sum()), int(copied.sum()), int(untouched.sum())


@functools.lru_cache(maxsize=None)
def _shape1_layer(name):
    """A shape-1 layer with as many images as its dense and its list case need: (problem, n dense, (n list, count1, count0))."""
    cin, cout, hw, ksize, groups = cc.SHAPE1_LAYERS[name]
    n_dense = cc.smallest_n_for_shape(1, cin, cout, hw, groups, _n_simd(), cc.N_SHAPES)
    plan = cc.list_shape1_plan(cout, hw, groups, _n_simd())
    assert n_dense is not None and n_dense <= 64 and plan is not None and plan[0] <= 64, (name, n_dense, plan)
    return _Conv(len(name), max(n_dense, plan[0]), cin, cout, hw, hw, ksize, groups), n_dense, plan


@pytest.mark.parametrize("name", list(cc.SHAPE1_LAYERS))
def test_dense_conv_on_both_sides_of_the_switch_to_shape_1(name):
    """(a) conv2 (5x5) and conv3 (3x3) at the smallest image count that picks the 32 x 96 tile, and at one image less (64 x 32)."""
    p, n1, _plan = _shape1_layer(name)
    cout_g = p.cout // p.groups
    assert cc.conv_pick_shape(n1 * p.h * p.w, cout_g, p.groups, _n_simd()) == 1
    worst = p.check_dense(n1)
    print("%s: dense shape 1 at n = %d (%d SIMDs), worst error %.3f of the tolerance" % (name, n1, _n_simd(), worst))
    if n1 > 1:
        below = cc.conv_pick_shape((n1 - 1) * p.h * p.w, cout_g, p.groups, _n_simd())
        assert below != 1
        worst = p.check_dense(n1 - 1)
        print("%s: dense shape %d at n = %d, worst error %.3f of the tolerance" % (name, below, n1 - 1, worst))


@pytest.mark.parametrize("name", list(cc.SHAPE1_LAYERS))
def test_listed_conv_on_both_sides_of_the_switch_to_shape_1(name):
    """(g) list mode against fp64 at the smallest listed count for which the workgroups pick the 32 x 96 tile, and one pixel below it;
    conv2 without a background (its consumer reads it), conv3 with one, as the network calls them."""
    p, _n1, (n, count1, count0) = _shape1_layer(name)
    cout_g, mall = p.cout // p.groups, n * p.h * p.w
    assert cc.conv_pick_shape(count1, cout_g, p.groups, _n_simd(), cc.LIST_SHAPES) == 1
    assert cc.conv_pick_shape(count0, cout_g, p.groups, _n_simd(), cc.LIST_SHAPES) == 0
    assert cc.list_is_followed(count1, mall) and cc.list_is_followed(count0, mall)
    rng = np.random.default_rng(count1)
    for count in (count1, count0):
        active = np.sort(rng.choice(mall, count, replace=False))
        done = p.check_list(active, n=n, background=p.ksize == 3)
        assert done[0] == count
    print("%s: list mode at n = %d (%d pixels, %d SIMDs): shape 1 at %d listed pixels, shape 0 at %d" % (name, n, mall, _n_simd(), count1, count0))


def test_dense_conv_k_loop_tail():
    """(b) 5x5 with 16, 32 and 64 input channels per group: Q = 25 * cin_g / 8 leaves two, one and two octets behind the triples."""
    for i, (name, n, cin, cout, h, w, groups) in enumerate(cc.CONV_TAIL_CASES):
        assert cc.conv_q(5, cin // groups) % 3 in (1, 2), name
        _Conv(100 + i, n, cin, cout, h, w, 5, groups).check_dense()


def test_dense_conv_grid_sweep():
    """(c) 3x3, 16 input channels per group: one to six channel tiles (odd counts take eight pixel ranges, even ones four per half) x
    pixel counts 1 .. 1,001 on non-square and one-row / one-column images.  One launch each, into NaN."""
    worst = 0.0
    for ci, (_cname, cout, groups) in enumerate(cc.GRID_CHANNELS):
        for ii, (_iname, n, h, w) in enumerate(cc.GRID_IMAGES):
            worst = max(worst, _Conv(1000 + 16 * ci + ii, n, cc.GRID_CIN * groups, cout, h, w, 3, groups).check_dense(variants=False))
    print("grid sweep: worst error %.3f of the tolerance" % worst)


def test_dense_conv_one_hot_on_a_non_square_image():
    """(d) one input element and one weight tap on a 5 x 9 image land on exactly one output element: a swap of H and W anywhere in
    the pixel arithmetic puts the 6.0 elsewhere (or loses it)."""
    n, cin, cout, h, w, groups = cc.ONE_HOT_SHAPE
    for name, b, c, y, x0, ky, kx, o in cc.ONE_HOT_PROBES:
        x = torch.zeros(n, cin, h, w, device=DEV)
        wt = torch.zeros(3, 3, cin // groups, cout, device=DEV)
        x[b, c, y, x0] = 3.0
        assert o // (cout // groups) == c // (cin // groups), name
        wt[ky, kx, c % (cin // groups), o] = 2.0
        out = torch.full((n, cout // 8, h, w, 8), float("nan"), device=DEV)
        got = kernels.from_c8(kernels.conv2d_same(kernels.to_c8(x), kernels.pack_conv_weights(wt), None, groups=groups, out=out))
        yy, xx = y - (ky - 1), x0 - (kx - 1)                 # the output position whose tap (ky, kx) reads (y, x0)
        assert 0 <= yy < h and 0 <= xx < w, name
        want = torch.zeros_like(got)
        want[b, o, yy, xx] = 6.0
        assert torch.equal(got, want), name


def test_listed_conv_at_the_tile_edges_and_the_copy_units():
    """(e) 338 pixels, listed counts 0, 1, 31 .. 33, 95 .. 97 with a background (every pixel written: NaN-filled buffer) and without
    (the unlisted pixels keep the sentinel); then 127, 128 and 129 pixels left to the background copy."""
    n, cin, cout, h, w, ksize, groups = cc.LIST_EDGE_LAYER
    p = _Conv(5, n, cin, cout, h, w, ksize, groups)
    mall = n * h * w
    rng = np.random.default_rng(8)
    for count in cc.LIST_EDGE_COUNTS:
        active = np.sort(rng.choice(mall, count, replace=False))
        assert p.check_list(active, background=True) == (count, mall - count, 0)
        assert p.check_list(active, background=False) == (count, 0, mall - count)
    for rest in cc.LIST_FILL_REMAINDERS:
        active = np.sort(rng.choice(mall, mall - rest, replace=False))
        assert p.check_list(active, background=True) == (mall - rest, rest, 0)


def test_listed_conv_follows_the_list_below_97_percent_only():
    """(f) 100 pixels, no background: at 96 listed pixels the four others keep the sentinel, at 97 and at 100 all are computed."""
    n, cin, cout, h, w, ksize, groups = cc.DENSE_RULE_LAYER
    p = _Conv(6, n, cin, cout, h, w, ksize, groups)
    rng = np.random.default_rng(9)
    for name, count, followed in cc.DENSE_RULE_COUNTS:
        active = np.sort(rng.choice(100, count, replace=False))
        assert p.check_list(active, background=False) == ((count, 0, 100 - count) if followed else (100, 0, 0)), name


def test_listed_conv_stops_at_live():
    """(h) six images, the lists cover the leading live ones: images at or behind live keep the sentinel, with a background and
    without; a live beyond the image count means all of them."""
    n, cin, cout, h, w, ksize, groups = cc.LIST_LIVE_LAYER
    p = _Conv(7, n, cin, cout, h, w, ksize, groups)
    hw = h * w
    rng = np.random.default_rng(10)
    for live in cc.LIST_LIVE_VALUES:
        covered = min(live, n)
        count = (2 * covered * hw) // 5
        active = np.sort(rng.choice(covered * hw, count, replace=False))
        assert p.check_list(active, background=True, live=live) == (count, covered * hw - count, (n - covered) * hw)
        assert p.check_list(active, background=False, live=live) == (count, 0, n * hw - count)
    full = np.arange(hw)                                      # one live image, listed in full: computed whole, nothing behind it
    assert p.check_list(full, background=True, live=1) == (hw, 0, (n - 1) * hw)


def test_conv_refuses_shapes_it_has_no_kernel_for():
    """Truthful buffers, unsupported shapes: 8 input channels per group, 32 output channels per group, a 7x7 filter."""
    for cin, cout, ksize in ((8, 64, 3), (16, 32, 3), (16, 64, 7)):
        x = torch.zeros(1, cin // 8, 6, 5, 8, device=DEV)
        wp = torch.zeros(ksize, ksize, cin // 8, cout, 8, device=DEV)
        with pytest.raises(_lib.SvxError):
            kernels.conv2d_same(x, wp)


# ---- fully connected ----
class _Fc:
    def __init__(self, m, n, k):
        rng = np.random.default_rng(m + n + k)
        self.m, self.n, self.k = m, n, k
        self.x = _dev(rng.standard_normal((m, k)).astype(np.float32))
        self.w = _dev((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32))
        self.b = _dev(rng.standard_normal(n).astype(np.float32))
        self.want = self.x.double() @ self.w.double().t() + self.b.double()
        self.wp = kernels.pack_fc_weights(self.w)

    def run(self, relu=False, live=None, fill=float("nan"), x=None, bias=None):
        out = torch.full((self.m, self.n), fill, dtype=torch.float32, device=DEV)
        y = kernels.fc_bias_act(self.x if x is None else x, self.wp, self.b if bias is None else bias, relu=relu, out=out,
                                live=None if live is None else _int1(live))
        assert y.data_ptr() == out.data_ptr()
        return y

    def check(self):
        got = self.run()
        err, tol = float((got.double() - self.want).abs().max()), FC_TOL * float(self.want.abs().max())
        assert err < tol, ((self.m, self.n, self.k), err, tol)
        assert torch.equal(self.run(relu=True), got.clamp_min(0))
        return got

    def check_one_hot(self):
        """One element of the last row: transposition and packing mix-ups, and a last row that leaks or is lost."""
        probe = torch.zeros(self.m, self.k, device=DEV)
        probe[self.m - 1, self.k - 3] = 2.0
        hot = self.run(x=probe, bias=torch.zeros(self.n, device=DEV))
        ref = torch.zeros(self.m, self.n, device=DEV)
        ref[self.m - 1] = 2.0 * self.w[:, self.k - 3]
        assert torch.equal(hot, ref), (self.m, self.n, self.k)


def test_fc_every_tail_length_in_every_instantiation():
    """(i) one split of 24 .. 29 octets: the unrolled body runs four times and the tail 0 .. 5 stages, in <1,1>, <1,2> and <2,2>."""
    for name, m, n in cc.FC_TAIL_MN:
        assert "<%d,%d>" % cc.fc_instantiation(m, n) == name
        left = set()
        for k in cc.FC_TAIL_K:
            q = cc.fc_q_lengths(m, n, k)
            assert len(q) == 1
            left.add(q[0] % cc.FC_RING)
            p = _Fc(m, n, k)
            p.check()
            p.check_one_hot()
        assert left == {0, 1, 2, 3, 4, 5}, name


def test_fc_row_tiles_and_row_edges():
    """(j) <1,2> with two and three row tiles (m > 64, n not a multiple of 64), and m = 32, 33, 64, 65 across the switch between the
    three instantiations; the one-hot probe sits in row m - 1."""
    seen = set()
    for name, m, n, k in cc.FC_ROW_TILE_CASES:
        seen.add((cc.fc_instantiation(m, n), cc.fc_row_tiles(m)))
        p = _Fc(m, n, k)
        p.check()
        p.check_one_hot()
    assert {((1, 2), 2), ((1, 2), 3), ((1, 1), 1), ((1, 2), 1), ((2, 2), 2)} <= seen


def test_fc_stops_at_live():
    """(k) rows behind live keep the sentinel bit for bit; rows in front are bit-identical to the run without live (DeviceStage gathers
    them into rows computed without it)."""
    m, k = cc.FC_LIVE_M, cc.FC_LIVE_K
    for n in cc.FC_LIVE_N:
        p = _Fc(m, n, k)
        full = p.check()
        for live in cc.FC_LIVE_VALUES:
            rows = min(live, m)
            got = p.run(live=live, fill=SENTINEL)
            assert torch.equal(got[:rows], full[:rows]), (n, live)
            assert torch.equal(got[rows:], torch.full_like(got[rows:], SENTINEL)), (n, live)


# ---- pooling + LRN ----
def _pool_into_nan(x, bias, radius, alpha, beta, k):
    """svx_bias_relu_pool_lrn_live through the C ABI, so that the output buffer can be handed in NaN-filled (the wrapper allocates it)."""
    n, o, h, w, _e = x.shape
    y = torch.full((n, o, (h - 3) // 2 + 1, (w - 3) // 2 + 1, 8), float("nan"), dtype=torch.float32, device=DEV)
    rc = _lib.load().svx_bias_relu_pool_lrn_live(x.data_ptr(), bias.data_ptr(), y.data_ptr(), n, o * 8, h, w, 1, radius, alpha, beta, k, None, None,
                                                 None, ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    _lib.check(rc, "svx_bias_relu_pool_lrn")
    return y


def test_pool_lrn_parameters_and_odd_geometry():
    """(l) radius 0, 1, 5 and C (the window clamps at both channel ends), beta 0.75 (the rsqrt form) and 0.5 / 1.0 (powf), k 1 and 2, on
    a single pooled pixel, even heights and widths and a width beyond 32, inputs of scale 30 and 3,000; against the NumPy restatement
    on float64.  An all-negative input gives exactly 0."""
    for si, (sname, n, c, h, w) in enumerate(cc.POOL_SHAPES):
        rng = np.random.default_rng(40 + si)
        unit = rng.standard_normal((n, c, h, w))
        b = rng.standard_normal(c).astype(np.float32)
        for scale in cc.POOL_SCALES:
            x = (unit * scale).astype(np.float32)
            xc, bt = kernels.to_c8(_dev(x)), _dev(b)
            pooled = alexnet_ref._max_pool_3x3s2_valid(np.ascontiguousarray(np.maximum(x.astype(np.float64).transpose(0, 2, 3, 1) + b.astype(np.float64), 0)))
            for pname, radius, alpha, beta, k in cc.POOL_PARAMS:
                radius = c if radius is None else radius
                y = _pool_into_nan(xc, bt, radius, alpha, beta, k)
                assert torch.equal(y, kernels.bias_relu_pool_lrn(xc, bt, lrn=True, radius=radius, alpha=alpha, beta=beta, k=k))     # the wrapper passes them on
                got = kernels.from_c8(y).cpu().numpy()
                want = alexnet_ref._lrn(np.ascontiguousarray(pooled), radius=radius, alpha=alpha, beta=beta, bias=k).transpose(0, 3, 1, 2)
                assert got.shape == want.shape
                assert np.allclose(got, want, rtol=1e-5, atol=1e-6), (sname, scale, pname, float(np.nanmax(np.abs(got - want))))
        neg = kernels.to_c8(_dev((-np.abs(unit) * 30 - 1).astype(np.float32)))
        for pname, radius, alpha, beta, k in cc.POOL_PARAMS:
            y = _pool_into_nan(neg, _dev(-np.abs(b)), c if radius is None else radius, alpha, beta, k)
            assert torch.equal(y, torch.zeros_like(y)), (sname, pname)


# ---- last layer ----
def test_fc8_softmax_ties_large_logits_and_live():
    """(m) 1, 64 and 65 rows.  Classes 1 and 3 share a weight row and a bias, so their logits are equal bit for bit: where they are the
    largest the class is 1, the first.  One row has logits near +300 and -300, where exp() without the shift overflows: its softmax is
    finite and sums to 1.  Logits against an fp64 product (the fc tolerance), the softmax against fp64 on the returned logits."""
    rng = np.random.default_rng(12)
    w = (rng.standard_normal((5, 4096)) * 0.03).astype(np.float32)
    b = rng.standard_normal(5).astype(np.float32)
    w[3], b[3] = w[1], b[1]
    unit = [w[j].astype(np.float64) / float(w[j].astype(np.float64) @ w[j].astype(np.float64)) for j in range(5)]
    for n in cc.FC8_ROWS:
        x = rng.standard_normal((n, 4096)).astype(np.float32)
        tie_row, big_row = n - 1, n // 2
        x[tie_row] = (8.0 * unit[1]).astype(np.float32)                        # classes 1 and 3 at about 8 + bias, the others near their bias
        if n > 1:
            x[big_row] = (300.0 * (unit[0] - unit[2])).astype(np.float32)      # class 0 near +300, class 2 near -300
        out = torch.full((n, 12), float("nan"), device=DEV)
        got = kernels.fc8_softmax(_dev(x), _dev(w), _dev(b), out=out).cpu().numpy()
        logits = x.astype(np.float64) @ w.T.astype(np.float64) + b
        assert np.abs(got[:, 6:11] - logits).max() < FC_TOL * np.abs(logits).max()
        assert np.array_equal(got[:, 11], np.zeros(n, np.float32))
        assert got[tie_row, 7] == got[tie_row, 9] == got[tie_row, 6:11].max() and got[tie_row, 5] == 1.0
        assert got[tie_row, 1] == got[tie_row, 3]
        mine = got[:, 6:11].astype(np.float64)
        assert np.array_equal(got[:, 5].astype(int), mine.argmax(1))           # (argmax: the first maximal index)
        e = np.exp(mine - mine.max(1, keepdims=True))
        assert np.abs(got[:, :5] - e / e.sum(1, keepdims=True)).max() < 1e-6
        assert np.isfinite(got).all() and np.abs(got[:, :5].astype(np.float64).sum(1) - 1).max() < 1e-6
        if n > 1:
            assert logits[big_row, 0] > 250 and logits[big_row, 2] < -250
            assert got[big_row, 5] == 0.0 and got[big_row, 0] == 1.0 and got[big_row, 2] == 0.0
        for live in sorted({1, n - 1, n, n + 5} - {0}):
            kept = torch.full((n, 12), SENTINEL, device=DEV)
            part = kernels.fc8_softmax(_dev(x), _dev(w), _dev(b), out=kept, live=_int1(live)).cpu().numpy()
            rows = min(live, n)
            assert np.array_equal(part[:rows], got[:rows]) and np.array_equal(part[rows:], np.full((n - rows, 12), SENTINEL, np.float32)), (n, live)
