"""GPU test (-m gpu) of svx_fc8_tail_live: fc7's ordered reduce + fc8 + softmax + the gather through inv in one launch must write the
packed rows of the separate launches (svx_fc_bias_act_live's reduce, svx_fc8_softmax_live, svx_gather_rows), bit for bit.

Random partial sums [splits, m, 4096] with splits 1 and 4, m = 1 / 64 / 256, live = 1, m / 2 and m (at least 1), inv drawn from the
live rows so that rows repeat and some are never asked for.  The reduce of the separate path is restated with float32 tensor adds
in the kernel's order (bias, then split 0, 1, ...; IEEE adds, nothing to contract) and that restatement is itself held against
fc_reduce_kernel on a real fc7 launch in the second test, which also runs the whole chain both ways."""
import numpy as np
import pytest
import torch

from svision_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7777.25


def _int1(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def _ordered_reduce(part, bias):
    v = bias.clone().expand(part.shape[1], -1).contiguous()
    for s in range(part.shape[0]):
        v = v + part[s]
    return v.clamp_min(0)


@pytest.fixture(scope="module")
def fc8():
    g = torch.Generator(device="cpu").manual_seed(8)
    w = (torch.randn(5, 4096, generator=g) / 64).to(DEV)
    return w, torch.randn(5, generator=g).to(DEV), torch.randn(4096, generator=g).to(DEV)


@pytest.mark.parametrize("splits", [1, 4])
@pytest.mark.parametrize("m", [1, 64, 256])
def test_fused_tail_equals_reduce_fc8_gather(fc8, m, splits):
    w8, b8, b7 = fc8
    g = torch.Generator(device="cpu").manual_seed(100 * m + splits)
    part = torch.randn(splits, m, 4096, generator=g).to(DEV)
    x7 = _ordered_reduce(part, b7)
    for live in sorted({1, max(1, m // 2), m}):
        inv = torch.randint(0, live, (m,), generator=g, dtype=torch.int32).to(DEV)
        inv[m - 1] = live - 1                                    # the last live row is asked for, by the last record
        assert m == 1 or len(set(inv.tolist())) < m              # rows repeat
        packed = kernels.fc8_softmax(x7, w8, b8, out=torch.full((m, 12), SENTINEL, device=DEV), live=_int1(live))
        want = kernels.gather_rows(packed, inv)
        out = torch.full((m, 12), SENTINEL, device=DEV)
        got = kernels.fc8_tail(part, b7, w8, b8, inv, out=out, live=_int1(live))
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(got, want), (m, splits, live)


def test_fused_tail_on_a_real_fc7_launch(fc8):
    """fc7 at m = 256 (4 splits) and m = 64: fc_partial leaves the sums fc_bias_act reduces (same rows, bit for bit), and the chain
    through the fused tail equals the chain of separate launches for live below, at and above the narrow tiles' limits."""
    w8, b8, b7 = fc8
    g = torch.Generator(device="cpu").manual_seed(77)
    w7 = kernels.pack_fc_weights((torch.randn(4096, 4096, generator=g) / 64).to(DEV))
    for m in (64, 256):
        x = torch.randn(m, 4096, generator=g).to(DEV)
        for live in sorted({1, 32, 41, 64, m}):
            lv = _int1(live)
            inv = torch.randint(0, live, (m,), generator=g, dtype=torch.int32).to(DEV)
            x7 = kernels.fc_bias_act(x, w7, b7, relu=True, live=lv)
            part = kernels.fc_partial(x, w7, live=lv)
            assert m != 256 or part.shape[0] == 4
            assert torch.equal(_ordered_reduce(part, b7)[:live], x7[:live]), (m, live)
            want = kernels.gather_rows(kernels.fc8_softmax(x7, w8, b8, live=lv), inv)
            got = kernels.fc8_tail(part, b7, w8, b8, inv, live=lv)
            assert torch.equal(got, want), (m, live)
