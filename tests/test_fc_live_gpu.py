"""GPU test (-m gpu) of svx_fc_bias_act_live where its wave tile follows the live count: a launch of more than 64 rows takes one
32 x 32 wave per neuron tile and split up to 32 live rows, two of them up to 64 and the tile of m beyond (svision_amd/csrc/svx_fc.hip
fc_splitk_live_kernel); up to 64 rows it is the dense kernel with a row limit.

Shapes: n = 96 is no multiple of 64 (the wide tile is 32 x 64 there), the others take 64 x 64; k = 192 / 392 / 776 give at most 1 / 2 / 4
splits of 24, 24 + 25 and 24 + 24 + 24 + 25 octets, so the weight ring's prologue, its unrolled body and its tail stages all run; m = 33 .. 256 puts one to four row tiles behind the first, live = 0 .. m crosses
every regime switch.

Rows in front of live: bit for bit the dense call's (live=None: the path the existing suite holds against the oracle), and within the
project's fc tolerance (2e-5 of the largest magnitude) of a float64 x @ W^T + b.  Rows at and behind live: the sentinel they held --
the parent's kernels write none of them (fc_reduce_kernel returns for such a row), pinned here."""
import numpy as np
import pytest
import torch

from svision_amd import kernels

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FC_TOL = 2e-5
SENTINEL = -7777.25                  # finite, negative (no ReLU output), exactly representable
KS = (192, 392, 776)
MS = (33, 64, 65, 129, 256)
LIVES = (0, 1, 31, 32, 33, 63, 64, 65)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("n", [32, 64, 96, 128])
def test_fc_live_rows_equal_dense_rows(n):
    worst = 0.0
    for k in KS:
        rng = np.random.default_rng(1000 * n + k)
        w = _dev((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32))
        b = _dev(rng.standard_normal(n).astype(np.float32))
        wp = kernels.pack_fc_weights(w)
        x_all = _dev(rng.standard_normal((max(MS), k)).astype(np.float32))
        for m in MS:
            x = x_all[:m].contiguous()
            want = x.double() @ w.double().t() + b.double()
            tol = FC_TOL * float(want.abs().max())
            for relu in (False, True):
                dense = kernels.fc_bias_act(x, wp, b, relu=relu)
                ref = want.clamp_min(0) if relu else want
                err = float((dense.double() - ref).abs().max())
                assert err < tol, ("dense", n, k, m, relu, err, tol)
                for live in sorted({min(v, m) for v in LIVES + (m,)}):
                    out = torch.full((m, n), SENTINEL, dtype=torch.float32, device=DEV)
                    got = kernels.fc_bias_act(x, wp, b, relu=relu, out=out, live=torch.tensor([live], dtype=torch.int32, device=DEV))
                    assert got.data_ptr() == out.data_ptr()
                    assert torch.equal(got[:live], dense[:live]), (n, k, m, relu, live)
                    assert torch.equal(got[live:], torch.full_like(got[live:], SENTINEL)), (n, k, m, relu, live)
                    if live:
                        err = float((got[:live].double() - ref[:live]).abs().max())
                        worst = max(worst, err / tol)
                        assert err < tol, (n, k, m, relu, live, err, tol)
    print("n = %d: worst error %.3f of the tolerance" % (n, worst))


def test_fc_live_count_above_the_launch_is_the_launch():
    """A count larger than m (a stale buffer) is clipped to m in every regime of the kernel."""
    n, k = 64, 392
    rng = np.random.default_rng(7)
    w = _dev((rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32))
    b = _dev(rng.standard_normal(n).astype(np.float32))
    wp = kernels.pack_fc_weights(w)
    for m in (65, 129):
        x = _dev(rng.standard_normal((m, k)).astype(np.float32))
        dense = kernels.fc_bias_act(x, wp, b, relu=True)
        got = kernels.fc_bias_act(x, wp, b, relu=True, live=torch.tensor([m + 500], dtype=torch.int32, device=DEV))
        assert torch.equal(got, dense), m
