"""GPU test (-m gpu) of svx_image_dedup's two forms: one workgroup that keys, finds first occurrences and compacts a launch of at
most 1,024 records (dedup_small_kernel, block = the launch rounded up to whole waves), and first_kernel + compact_kernel beyond.

Sizes: 1 record; 63 / 64 / 65 around one wave; 255 / 256 / 257 around the key tile of the two-kernel form; 1,023 / 1,024 full
blocks; 1,025 is the first size of the two-kernel form.  Record sets: all equal (one live row), all distinct (live = n: every lane
walks every key in front of it) and a period of 256 (every record equals the one exactly 256 before it: a duplicate whose first
occurrence lies in another wave, and in another key tile of the two-kernel form).  unique, inv, live and keys against a NumPy
first-occurrence model on the Python restatement of the key; the two forms against each other on the same records."""
import functools

import numpy as np
import pytest
import torch

from svision_amd import kernels
from tests import datagen
from tests.test_image_memo_cpu import keys_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


@functools.lru_cache(maxsize=None)
def _distinct_records(n=max(SIZES)):
    recs = datagen.random_records(4 * n + 64, seed=77, hostile=False)
    _u, first = np.unique(keys_of(recs), axis=0, return_index=True)
    assert first.size >= n
    return recs[np.sort(first)[:n]]


def _records(kind, n):
    if kind == "equal":
        return np.repeat(_distinct_records()[5:6], n, axis=0)
    if kind == "distinct":
        return _distinct_records()[:n].copy()
    return _distinct_records()[np.arange(n) % 256].copy()               # "period": record i == record i - 256


def _model(recs):
    """-> (unique [n,12], inv [n], live, keys [n,4]) of the first-occurrence compaction in input order."""
    keys = keys_of(recs)
    row, inv, order = {}, [], []
    for i, k in enumerate(map(tuple, keys)):
        if k not in row:
            row[k] = len(row)
            order.append(i)
        inv.append(row[k])
    unique = np.repeat(recs[:1], recs.shape[0], axis=0)      # the rows behind the distinct ones repeat record 0
    unique[:len(order)] = recs[order]
    return unique, np.asarray(inv, np.int32), len(order), keys


def _run(recs, keys):
    got = kernels.image_dedup(torch.from_numpy(np.ascontiguousarray(recs, np.int32)).to(DEV), keys=keys)
    return [t.cpu().numpy() for t in got]


@pytest.mark.parametrize("kind", ["equal", "distinct", "period"])
@pytest.mark.parametrize("n", SIZES)
def test_dedup_equals_first_occurrence_model(n, kind):
    recs = _records(kind, n)
    want_unique, want_inv, want_live, want_keys = _model(recs)
    assert want_live == {"equal": 1, "distinct": n, "period": min(n, 256)}[kind]
    for with_keys in (True, False):
        got = _run(recs, with_keys)
        assert int(got[2][0]) == want_live
        assert np.array_equal(got[1], want_inv)
        assert np.array_equal(got[0], want_unique)
        if with_keys:
            assert np.array_equal(got[3].view(np.uint32), want_keys)


@pytest.mark.parametrize("kind", ["equal", "distinct", "period"])
def test_one_workgroup_form_agrees_with_the_two_kernel_form(kind):
    """1,025 records (two kernels) against their first 1,024 (one workgroup): every record in front of the last has no other
    first occurrence with the last one there, so inv and keys of the prefix are the same and so are the prefix's unique rows."""
    recs = _records(kind, 1025)
    u2, inv2, live2, keys2 = _run(recs, True)
    u1, inv1, live1, keys1 = _run(recs[:1024], True)
    assert np.array_equal(inv2[:1024], inv1) and np.array_equal(keys2[:1024], keys1)
    assert np.array_equal(u2[:int(live1[0])], u1[:int(live1[0])])
    assert int(live2[0]) - int(live1[0]) == (1 if kind == "distinct" else 0)
