"""--hash on the device, a window at a time: the compacted read-back (svx_hash_pack_hits), launches cut by a byte budget, the
asynchronous handle, the two-phase collection and the helpers' requests to the owner.  The yardstick is the host aligner
(tests/hashcases.raw_hit_lists) and the reference's own run (tests/golden/hash_collect.expected.json), never the device."""
import json
import os

import numpy as np
import pytest

from tests import hashcases as hc
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, W = 2, 2                                       # the overflow case's parameters: every job of a batch shares them

_WANT = {}


def want(ref, seq, k=K, w=W):
    """The host aligner's two lists of a pair (once per process); None where a list exceeds the kernel's capacity."""
    key = (ref, seq, k, w)
    if key not in _WANT:
        a, b = hc.raw_hit_lists(ref, seq, k, w)
        _WANT[key] = None if max(len(a), len(b)) > 4 * len(ref) + 64 else (a, b)
    return _WANT[key]


def shaped_batch(n):
    """n (ref, seq) pairs at k = 2, window = 2 out of the catalogue's tiny cases: lists without rows at the first, a middle
    and the last position, A without B and B without A next to each other, the overflowing job between two with hits."""
    c = hc.by_name()
    under, over, both = c["b/hand/k2w2/repeat-under-cap"], c[hc.OVERFLOW], c["b/hand/k2w2/both-strands"]
    if n == 1:
        return [(under.ref, under.seq)]
    empty = [c["g/both-empty/k2w2"], c["g/both-short/k2w2"], c["g/empty-window/k2w2"]]
    a_only = (both.ref, c["g/empty-piece/k2w2"].seq)                       # a window with a hit of its own, nothing to place
    b_only = (c["b/hand/k3w3/repeat"].ref, c["b/hand/k3w3/repeat"].seq)
    fill = [x for x in hc.all_cases() if (x.name.startswith("g/") or x.name.startswith("b/hand/")) and len(x.ref) <= 80 and len(x.seq) <= 320]
    assert len(fill) > 20
    pairs = [(fill[j % len(fill)].ref, fill[(j * 7) % len(fill)].seq if j % 5 == 0 else fill[j % len(fill)].seq) for j in range(n)]
    pairs[0] = (empty[0].ref, empty[0].seq)
    pairs[1], pairs[2] = a_only, b_only
    pairs[3], pairs[4], pairs[5] = (under.ref, under.seq), (over.ref, over.seq), (both.ref, both.seq)
    pairs[n // 2] = (empty[1].ref, empty[1].seq)
    pairs[-1] = (empty[2].ref, empty[2].seq)
    assert [bool(l) for l in want(*a_only)] == [True, False] and [bool(l) for l in want(*b_only)] == [False, True]
    assert want(over.ref, over.seq) is None and all(want(e.ref, e.seq) == ([], []) for e in empty)
    return pairs


def check(pairs, got, k=K, w=W):
    assert len(got) == len(pairs)
    for j, ((ref, seq), g) in enumerate(zip(pairs, got)):
        expect = want(ref, seq, k, w)
        if expect is None:
            assert g is None, j
        else:
            assert g is not None, j
            assert (g[0].tolist(), g[1].tolist()) == expect, j


@pytest.mark.parametrize("n", [1, 64, 65, 257, 1100])
def test_packed_lists_equal_host_aligner(n):
    """2 n lists through the prefix of svx_hash_pack_hits (one wave, one workgroup's chunk, several chunks), the first pack into
    an array of ONE row (so it is repeated with the size the offsets ask for): every job's lists are the host aligner's."""
    from svision_amd import kernels
    pairs = shaped_batch(n)
    packed = [(kernels.pack_bases(seq), kernels.pack_bases(ref)) for ref, seq in pairs]
    bases, desc = kernels.hash_job_arrays(packed)
    handle = kernels.hash_seeds_async(bases, desc, K, W, DEV, packed_rows=1)
    counts, row_off, rows = handle.result()
    assert handle.done() and handle.launches == 1
    check(pairs, kernels.hash_split_rows(desc, counts, row_off, rows))
    # the offsets: an exclusive prefix over the rows every list really has (none where it overflowed; the count still tells)
    cap = np.repeat(kernels.hash_hit_caps(desc), 2)
    kept = np.where(counts > cap, 0, counts)
    assert row_off.tolist() == np.concatenate([[0], np.cumsum(kept)]).tolist() and len(rows) == int(row_off[-1]) > 1
    if n > 1:
        assert counts[2 * 4:2 * 4 + 2].tolist() == [1, 1023] and (row_off[9] - row_off[8], row_off[10] - row_off[9]) == (1, 0)
    if n == 65:                                                           # room from the start: no second pack, the same lists
        check(pairs, kernels.hash_seeds(packed, K, W, DEV))


def test_budget_splits_do_not_change_results():
    """Ten jobs under a byte budget that cuts them into three or more launches over ONE scratch area (dirty from the launch
    before), forwards and backwards: the lists of the single launch, which are the host aligner's."""
    from svision_amd import kernels
    c = hc.by_name()
    names = ["a/k10w10/00-fwd", "g/inner-rc/k10w50", hc.CHUNK_EDGE, "a/k10w10/02-mix", "g/both-empty/k10w50", hc.ONE_Y,
             "a/k10w10/01-rc", "g/equal/k10w50", "b/hand/k2w50/run", "a/k10w10/03-novel"]
    pairs = [(c[n].ref, c[n].seq) for n in names]
    packed = [(kernels.pack_bases(seq), kernels.pack_bases(ref)) for ref, seq in pairs]
    one = kernels.hash_seeds(packed, 10, 50, DEV)
    check(pairs, one, 10, 50)
    assert sum(bool(len(r[1])) for r in one) >= 6
    budget = 700_000                                                     # a 1,500-base window: 262 KB of table + 194 KB of lists
    for order in (slice(None), slice(None, None, -1)):
        bases, desc = kernels.hash_job_arrays(packed[order])
        handle = kernels.hash_seeds_async(bases, desc, 10, 50, DEV, budget=budget, packed_rows=8)
        got = kernels.hash_split_rows(desc, *handle.result())
        assert handle.launches >= 3
        check(pairs[order], got, 10, 50)
        check(pairs[order], kernels.hash_seeds(packed[order], 10, 50, DEV, budget=budget), 10, 50)


def test_long_window_beside_small_jobs_through_the_handle():
    """A 20,000-base window (2,000-base piece) planted among 30 small jobs, through hash_seeds_async: the host aligner's lists."""
    from svision_amd import kernels
    c = hc.by_name()
    small = ([x for x in hc.sweep_cases() if x.k == 10] + [x for x in hc.degenerate_cases() if x.name.endswith("k10w50")]
             + [x for x in hc.tiny_cases() if x.name.startswith("b/hand/")])
    assert len(small) >= 30
    pairs = [(x.ref, x.seq) for x in small[:30]]
    pairs.insert(17, (c[hc.LARGE].ref, c[hc.LARGE].seq))
    assert len(pairs) == 31
    packed = [(kernels.pack_bases(seq), kernels.pack_bases(ref)) for ref, seq in pairs]
    bases, desc = kernels.hash_job_arrays(packed)
    handle = kernels.hash_seeds_async(bases, desc, 10, 50, DEV)
    while not handle.done():                                             # (polling, as the owner's loop does)
        pass
    got = kernels.hash_split_rows(desc, *handle.result())
    check(pairs, got, 10, 50)
    assert len(got[17][1]) >= 1 and handle.launches == 1


def test_refusals_of_the_batch_form():
    """What the wrapper refused before, it refuses: a 2,049-base piece; and a descriptor that points outside the bases."""
    from svision_amd import _lib, kernels
    long_piece = hc.by_name()[hc.TOO_LONG]
    with pytest.raises(_lib.SvxError):
        kernels.hash_seeds([(kernels.pack_bases(long_piece.seq), kernels.pack_bases(long_piece.ref))], 10, 50, DEV)
    with pytest.raises(_lib.SvxError):
        kernels.hash_seeds_async(np.zeros(100, np.uint8), np.array([[0, 50, 50, 51]], np.int64), 10, 50, DEV)
    assert kernels.hash_seeds([], 10, 50, DEV) == []
    assert kernels.hash_seeds_async(np.zeros(0, np.uint8), np.zeros((0, 4), np.int64), 10, 50, DEV).result()[1].tolist() == [0]


# ---- collection ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def expected():
    with open(os.path.join(helpers.GOLDEN, "hash_collect.expected.json")) as f:
        return [w for w in json.load(f)["windows"] if w["hash"]][0]


def _device_sample():
    from svision_amd.io import bam
    from svision_amd.sample import Sample
    table = bam.read_bam(os.path.join(helpers.GOLDEN, "hash_collect.bam"), with_seq=True)
    return Sample.from_table(table, helpers.load_golden_fasta("hash_collect.fa.gz"), 50, device=DEV)


@pytest.mark.parametrize("batch,calls_want", [("1", [51]), ("0", [1] * 51)])
def test_collection_is_one_executor_call_per_window(expected, monkeypatch, batch, calls_want):
    """detect_window --hash with the device scan and the device re-aligner == the reference's signatures and TSV; the executor
    is called once with the window's 51 jobs (SVX_HASH_BATCH=0: 51 times with one, as before)."""
    from svision_amd import kernels
    from svision_amd.collection.output_clusters import collect_pair_lines
    from svision_amd.collection.run_collection import detect_window
    monkeypatch.setenv("SVX_HASH_BATCH", batch)
    calls, orig = [], kernels.hash_seeds
    monkeypatch.setattr(kernels, "hash_seeds", lambda *a, **kw: (calls.append(len(a[0])), orig(*a, **kw))[1])
    sample = _device_sample()
    opts = helpers.default_options(min_support=3, hash=True)
    sigs, clusters = detect_window(opts, sample, "chrH", 0, 160_000)
    got = [[s.type, s.tstart, s.tend, s.qname, s.bkps, s.mechanism,
            [[a.q_start, a.q_end, a.ref_start, a.ref_end, bool(a.is_reverse)] for a in s.sorted_aligns]] for s in sigs]
    assert calls == calls_want
    assert got == expected["signatures"]
    assert "".join(p.text() for p in collect_pair_lines(clusters, opts)) == expected["tsv"]


@pytest.fixture(scope="module")
def net():
    from oracle import alexnet_ref
    from svision_amd.network.alexnet import AlexNet
    return AlexNet(alexnet_ref.random_params(seed=7), device=DEV)


@pytest.fixture(scope="module")
def streamed(net, expected):
    """The one-process streaming result of the window (its own collection runs the batch on the device)."""
    from svision_amd.pipeline import HotPath
    opts = helpers.default_options(min_support=3, batch_size=64, hash=True, bam_path="<resident>")
    res = list(HotPath(_device_sample(), opts, net, device=DEV, n_streams=2).run_windows([("chrH", 0, 160_000)]))[0]
    assert "".join(ln.text() for ln in res.lines) == expected["tsv"]
    return res.vcf, res.scores, res.n_sites, res.n_images


@pytest.mark.parametrize("batch", ["1", "0"])
def test_helpers_ask_the_owner(net, expected, streamed, monkeypatch, batch):
    """Two helpers: the one that collects the window sends its 51 jobs to the owner, which answers from the device; TSV and VCF
    are the one-process run's and the reference's TSV.  SVX_HASH_BATCH=0: no request, the same outputs."""
    from svision_amd.pipeline import PooledHotPath
    monkeypatch.setenv("SVX_HASH_BATCH", batch)                            # (the helpers are forked below: they inherit it)
    opts = helpers.default_options(min_support=3, batch_size=64, hash=True, bam_path="<resident>")
    hp = PooledHotPath(_device_sample(), opts, net, device=DEV, n_workers=2, n_streams=2, want_tsv=True)
    try:
        res = list(hp.run_windows([("chrH", 0, 160_000)]))[0]
    finally:
        hp.close()
    assert res.tsv == expected["tsv"]
    assert (res.vcf, res.scores, res.n_sites, res.n_images) == streamed
    prof = hp.owner_profile
    if batch == "1":
        assert prof["hash.jobs"] == 51 and prof["hash.requests"] >= 1 and prof["hash.launches"] >= 1 and prof["hash.wait_s"] > 0
    else:
        assert prof["hash.jobs"] == 0 and prof["hash.requests"] == 0
