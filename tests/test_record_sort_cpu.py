"""CPU: what the device record sort is asked for (svision_amd/ingest_sort.py's planning helpers) and the oracle its GPU tests lean on
(tests/sortcases.py).  The helpers against np.lexsort on crafted keys; then record-shuffled copies of tests/golden/collect_small.bam
(1,491 records, 2 references, hundreds of key ties): the host reader decodes such a file in FILE order, and its table reordered by
the oracle is the table of the stably sorted file."""
import os
import re

import numpy as np
import pytest

from svision_amd import ingest_sort as isort
from svision_amd import kernels
from svision_amd.io import bam
from tests import helpers, sortcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def crafted(n_ref, max_len, n=4000, seed=1):
    """tid in -1 .. n_ref - 1 and pos in -1 .. max_len - 1, the extremes present, every key several times."""
    rng = np.random.default_rng(seed)
    tid = rng.integers(-1, n_ref - 1, n, endpoint=True).astype(np.int32)
    pos = rng.choice(np.asarray([-1, 0, 1, 254, 255, 256, max_len // 2, max_len - 2, max_len - 1], np.int64), n).astype(np.int32)
    tid[:4], pos[:4] = (-1, -1, n_ref - 1, 0), (-1, max_len - 1, max_len - 1, -1)
    return tid, pos


@pytest.mark.parametrize("n_ref,max_len", [(1, 1000), (1, (1 << 31) - 2), (2, 420_000), (3366, 248_956_422), (3366, (1 << 31) - 2)])
def test_key_and_digit_plan_against_lexsort(n_ref, max_len):
    """sort_key orders as np.lexsort over (tid with -1 last, pos + 1, input index); the packed key keeps that order in
    pos_bits + bit_length(n_ref) bits; and the planned 8-bit passes, lowest digit first and each one stable, arrive at it."""
    tid, pos = crafted(n_ref, max_len)
    want = np.lexsort((np.arange(tid.size), pos.astype(np.int64) + 1, np.where(tid < 0, n_ref, tid)))
    key = isort.sort_key(tid, pos, n_ref)
    assert key.dtype == np.uint64 and np.array_equal(key, sortcases.key(tid, pos, n_ref))
    assert np.array_equal(np.argsort(key, kind="stable"), want)
    assert int(key.max()) == (n_ref << 32) | max_len             # tid -1 at the largest position: behind every reference
    pos_bits = isort.pos_bits_for([7, max_len, 12])
    assert pos_bits == (max_len + 1).bit_length() and pos_bits <= 32
    assert isort.pos_bits_for([100], max_pos=70_000) == 17 and isort.pos_bits_for([]) == 1
    for bits in (pos_bits, 32):                                 # 32 must also work
        packed = isort.packed_key(tid, pos, n_ref, bits)
        assert int(packed.max()) < 1 << (bits + n_ref.bit_length())
        assert np.array_equal(np.argsort(packed, kind="stable"), want)
        plan = isort.digit_plan(n_ref, bits)
        assert plan == [8 * p for p in range(len(plan))] and 8 * len(plan) >= bits + n_ref.bit_length() > 8 * (len(plan) - 1)
        rows = np.arange(tid.size)
        for shift in plan:
            digit = (packed[rows] >> np.uint64(shift)) & np.uint64(255)
            rows = rows[np.argsort(digit, kind="stable")]
        assert np.array_equal(rows, want)
    assert isort.digit_plan(3366, 28) == [0, 8, 16, 24, 32] and isort.digit_plan(1, 1) == [0] and isort.digit_plan(0, 1) == [0]


def test_the_tile_is_the_headers():
    header = open(os.path.join(ROOT, "include", "svx.h")).read()
    assert int(re.search(r"#define\s+SVX_RECORD_SORT_TILE\s+(\d+)u", header).group(1)) == kernels.RECORD_SORT_TILE


@pytest.mark.parametrize("seed,sort_order", [(1, "unsorted"), (2, "queryname"), (3, None)])
def test_shuffled_copy_reordered_by_the_oracle_is_the_sorted_file(tmp_path, seed, sort_order):
    golden = os.path.join(helpers.GOLDEN, "collect_small.bam")
    src = bam.read_bam(golden, with_seq=True)
    n_ref = len(src.references)
    assert len(src) == 1491 and n_ref == 2
    assert len(src) - np.unique(sortcases.key(src.tid, src.pos, n_ref)).size == 365          # ties: stability is exercised
    path, sorted_path, want = sortcases.shuffled_files(golden, tmp_path, seed, sort_order)
    head = bam.read_bam_header(path)
    assert head.sort_order == sort_order and bam.read_bam_header(sorted_path).sort_order == "coordinate"
    # the host reader decodes the shuffled file in file order: the permutation the file was written with
    perm = np.random.default_rng(seed).permutation(len(src))
    got = bam.read_bam(path, with_seq=True)
    sortcases.assert_same_table(got, sortcases.reorder_table(src, perm), with_seq=True, what="file order")
    assert not np.array_equal(got.pos, src.pos)
    # reordered by the oracle it is the table of the stably sorted file ...
    o = sortcases.order(got.tid, got.pos, n_ref)
    sortcases.assert_same_table(sortcases.reorder_table(got, o), bam.read_bam(sorted_path, with_seq=True), with_seq=True, what="sorted file")
    sortcases.assert_same_table(want, bam.read_bam(sorted_path, with_seq=True), with_seq=True, what="expected table")
    # ... which is sorted, with every tie in the shuffled file's order (stability said without argsort)
    k = sortcases.key(got.tid, got.pos, n_ref)[o]
    assert (k[1:] >= k[:-1]).all() and (o[1:][k[1:] == k[:-1]] > o[:-1][k[1:] == k[:-1]]).all()
    # and it differs from the golden file only inside groups of equal keys
    assert np.array_equal(want.tid, src.tid) and np.array_equal(want.pos, src.pos)
    assert not np.array_equal(want.flag, src.flag) or not np.array_equal(want.cig_off, src.cig_off)
    # the product's own subset() agrees with the oracle's reordering
    sortcases.assert_same_table(got.subset(o), sortcases.reorder_table(got, o), what="subset")
