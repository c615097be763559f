"""GPU test of the image memo (-m gpu): svx_image_dedup keys every record exactly as the Python restatement of
tests/test_image_memo_cpu.py does, and the network run once per distinct image (memo on) gives every record the packed
row it gets without the memo, bit for bit -- eager and graph-replayed, at the launch sizes of the pipeline (64, 128, 256),
on the fixtures and on 10 k fuzzed records with planted duplicates, all-duplicate and all-distinct launches.  The rows
behind the live count never change the rows in front of it."""
import numpy as np
import pytest
import torch

from svision_amd import kernels
from svision_amd.network.alexnet import AlexNet
from svision_amd.pipeline import DeviceStage
from tests import datagen
from tests.test_image_memo_cpu import PAD, fixture_records, keys_of, planted

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (64, 128, 256)


@pytest.fixture(scope="module")
def net():
    from bench import random_weights
    return AlexNet(random_weights(4), device=DEV)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def _distinct(n, seed):
    """n records with n different keys."""
    recs = datagen.random_records(4 * n, seed=seed, hostile=False)
    _u, first = np.unique(keys_of(recs), axis=0, return_index=True)
    assert first.size >= n
    return recs[np.sort(first)[:n]]


def test_device_keys_equal_python_keys():
    img, col = fixture_records()
    for recs in (img, col, planted(seed=11, n=2000), np.asarray([PAD] * 7, np.int32)):
        _unique, _inv, _live, keys = kernels.image_dedup(_dev(recs), keys=True)
        assert np.array_equal(keys.cpu().numpy().view(np.uint32), keys_of(recs))


@pytest.mark.parametrize("n", [1, 63, 64, 256, 257, 1000, 3000])
def test_dedup_is_first_occurrence_compaction(n):
    recs = planted(seed=n, n=2 * n + 2)[:n]
    unique, inv, live = kernels.image_dedup(_dev(recs))
    keys = [tuple(k) for k in keys_of(recs)]
    first = {}
    for i, k in enumerate(keys):
        first.setdefault(k, len(first))
    want_inv = np.asarray([first[k] for k in keys])
    m = int(live.item())
    assert m == len(first)
    assert np.array_equal(inv.cpu().numpy(), want_inv)
    u = unique.cpu().numpy()
    seen, order = set(), []
    for i, k in enumerate(keys):
        if k not in seen:
            seen.add(k)
            order.append(i)
    assert np.array_equal(u[:m], recs[order])
    assert (u[m:] == recs[0]).all()


def _both(net, rec):
    a = net.predict_records_packed(rec, memo=False)
    b = net.predict_records_packed(rec, memo=True)
    return a, b


def _launches(n_per):
    """(name, records) launches of n_per rows: fuzz with planted duplicates, all duplicates, all distinct, fixtures, pads."""
    fuzz = planted(seed=21, n=10_000)
    img, col = fixture_records()
    out = [("fuzz%d" % i, fuzz[i:i + n_per]) for i in range(0, fuzz.shape[0] - n_per + 1, max(n_per, 10_000 // 12))]
    out.append(("all_dup", np.repeat(fuzz[:1], n_per, axis=0)))
    out.append(("all_pad", np.asarray([PAD] * n_per, np.int32)))
    out.append(("all_distinct", _distinct(n_per, seed=n_per)))
    for name, recs in (("image_small", img), ("collect_small", col)):
        tail = np.asarray([PAD] * ((-recs.shape[0]) % n_per), np.int32).reshape(-1, 12)
        full = np.concatenate([recs, tail])
        out += [("%s@%d" % (name, lo), full[lo:lo + n_per]) for lo in range(0, full.shape[0], n_per)]
    return out


@pytest.mark.parametrize("n_per", SIZES)
def test_memo_is_bit_identical_eager(net, n_per):
    for name, recs in _launches(n_per):
        a, b = _both(net, _dev(recs))
        assert torch.equal(a, b), name


def test_memo_is_bit_identical_on_the_whole_fuzz(net):
    """All 10 k fuzzed records, in launches of 2,000 (conv2's input at 10 k images would pass the 2 GB buffer limit)."""
    fuzz = planted(seed=21, n=10_000)
    for lo in range(0, fuzz.shape[0], 2000):
        a, b = _both(net, _dev(fuzz[lo:lo + 2000]))
        assert torch.equal(a, b), lo


def test_memo_is_bit_identical_graph_replay(net):
    """DeviceStage (captured graphs, launch sizes 256 / 128 / 64 with batch 64) with and without the memo."""
    fuzz = planted(seed=33, n=10_000)
    img, col = fixture_records()
    stages = {m: DeviceStage(net, 64, DEV, n_streams=2, use_graph=True, launch_batches=4, memo=m) for m in (False, True)}
    assert stages[True].sizes == [256, 128, 64]
    cases = [fuzz[:64 * 71], np.repeat(fuzz[:1], 448, axis=0), _distinct(448, seed=5), img, col]
    for recs in cases:
        tail = np.asarray([PAD] * ((-recs.shape[0]) % 64), np.int32).reshape(-1, 12)
        d_rec = _dev(np.concatenate([recs, tail]))
        outs = {}
        for m, st in stages.items():
            out = torch.empty((d_rec.shape[0], 6), dtype=torch.float32, device=DEV)
            st.run(d_rec, out)
            torch.cuda.synchronize()
            outs[m] = out
        assert torch.equal(outs[False], outs[True])


def test_rows_behind_the_live_count_never_change_the_rows_in_front(net):
    """The stage kernels with a live count: whatever the rows >= live hold, the rows < live come out the same."""
    recs = np.concatenate([_distinct(40, seed=8), datagen.random_records(216, seed=9, hostile=True)])
    rec_a = _dev(recs)
    rec_b = _dev(np.concatenate([recs[:40], datagen.random_records(216, seed=10, hostile=True)]))
    live = torch.tensor([40], dtype=torch.int32, device=DEV)

    def run(rec):
        x = net._convs(rec, live).reshape(rec.shape[0], 9216)
        x = kernels.fc_bias_act(x, net.fc6_w, net.fc6_b, relu=True, live=live)
        x = kernels.fc_bias_act(x, net.fc7_w, net.fc7_b, relu=True, live=live)
        return kernels.fc8_softmax(x, net.fc8_w, net.fc8_b, live=live)[:40]
    a, b = run(rec_a), run(rec_b)
    full = net.predict_records_packed(rec_a, memo=False)[:40]
    assert torch.equal(a, b) and torch.equal(a, full)
