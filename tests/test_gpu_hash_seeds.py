"""svx_hash_seeds (svision_amd/csrc/svx_hash.hip) beyond k = 10, window = 50 and 900 bases: the cases of tests/hashcases.py
(k 2..13, pieces up to the kernel's 2048 bases, windows up to 20,000 bases, overflowing hit lists, every symbol the packer
admits) against the host aligner's raw hit lists and the reference's final segments (tests/golden/hash_params.expected.json.gz)."""
import json
import os
import random

import numpy as np
import pytest

from tests import hashcases as hc
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_SINGLE = {}


def single(case, k=None, window=None):
    """The kernel's lists for one job alone in its launch (once per process); k / window default to the case's own."""
    from svision_amd import kernels
    k, window = k or case.k, window or case.window
    key = (case.name, k, window)
    if key not in _SINGLE:
        res = kernels.hash_seeds([(kernels.pack_bases(case.seq), kernels.pack_bases(case.ref))], k, window, DEV)[0]
        _SINGLE[key] = None if res is None else (res[0].tolist(), res[1].tolist())
    return _SINGLE[key]


def eligible():
    return [c for c in hc.all_cases() if hc.device_eligible(c)]


def test_raw_hit_lists_match_host_aligner():
    """Every eligible case alone in a launch: both lists equal the host aligner's, order included; None (overflow) for the
    overflow case and for no other."""
    cases = eligible()
    assert len(cases) == len(hc.all_cases()) - 4                         # all but the 2049-base piece and k = 14
    for c in cases:
        got = single(c)
        if c.name == hc.OVERFLOW:
            assert got is None
            continue
        assert got is not None, c.name
        want_a, want_b = hc.raw_hit_lists_of(c)
        assert got[0] == want_a, c.name
        assert got[1] == want_b, c.name


def test_final_segments_match_reference():
    """hashplot_unmapped_batch (one launch per (k, window)) + the host merge == the reference; what the kernel cannot take
    (overflow, 2049 bases, k = 14) == the reference through hashplot_unmapped's host fallback."""
    from svision_amd.segmentplot import run_hash_lineplot as rh
    want = hc.load_expected()
    groups = {}
    for c in eligible():
        groups.setdefault((c.k, c.window), []).append(c)
    assert len(groups) >= len(hc.SWEEP) + len(hc.TINY)
    for (k, window), cases in groups.items():
        got = rh.hashplot_unmapped_batch([(c.ref, c.seq) for c in cases], k, window, DEV)
        for c, segs in zip(cases, got):
            if c.name == hc.OVERFLOW:
                assert segs is None
                continue
            assert segs is not None, c.name
            assert hc.fmt(segs) == want[c.name]["segs"], c.name
    host_only = [c for c in hc.all_cases() if not hc.device_eligible(c)] + [hc.by_name()[hc.OVERFLOW]]
    assert sorted(c.name for c in host_only) == sorted([hc.TOO_LONG, hc.OVERFLOW] + [c.name for c in hc.k14_cases()])
    saved = rh.DEVICE
    try:
        rh.DEVICE = DEV
        for c in host_only:
            assert rh.hashplot_unmapped_batch([(c.ref, c.seq)], c.k, c.window, DEV) == [None], c.name
            main, segs = rh.hashplot_unmapped(c.ref, c.seq, c.k, c.window)
            assert main is None
            assert hc.fmt(segs) == want[c.name]["segs"], c.name
            assert hc.fmt(segs) == hc.fmt(rh._hashplot_host(c.ref, c.seq, c.k, c.window)), c.name
    finally:
        rh.DEVICE = saved


@pytest.mark.parametrize("k,window", [(2, 2), (10, 50), (13, 13)])
def test_batch_equals_single_launches(k, window):
    """All eligible sequences as ONE launch at (k, window), shuffled, an empty job first and last, the overflow job between
    the full-table job and a job with hits of its own; then the same batch reversed (the allocator hands back the dirty table
    and hit buffers): every job's lists equal those of the job alone in a launch, element for element."""
    from svision_amd import kernels
    cases = hc.by_name()
    first, last = cases["g/both-empty/k10w50"], cases["g/empty-piece/k10w50"]
    trio = [cases["c/piece2048/k2w2"], cases[hc.OVERFLOW], cases["b/hand/k2w2/repeat-under-cap"]]
    rest = [c for c in eligible() if c not in [first, last] + trio]
    random.Random(k * 100 + window).shuffle(rest)
    order = [first] + rest[:len(rest) // 2] + trio + rest[len(rest) // 2:] + [last]
    assert len(order) == len(eligible())
    want = [single(c, k, window) for c in order]
    if (k, window) == (2, 2):
        assert want[order.index(trio[1])] is None and len(want[order.index(trio[2])][1]) == 39
    assert sum(w is None for w in want) == (1 if (k, window) == (2, 2) else 0)
    assert sum(bool(w and w[1]) for w in want) >= 5
    packed = [(kernels.pack_bases(c.seq), kernels.pack_bases(c.ref)) for c in order]
    for jobs, expect in ((packed, want), (packed[::-1], want[::-1])):
        got = kernels.hash_seeds(jobs, k, window, DEV)
        assert len(got) == len(expect)
        for c, g, w in zip(order if jobs is packed else order[::-1], got, expect):
            if w is None:
                assert g is None, c.name
            else:
                assert g is not None, c.name
                assert (g[0].tolist(), g[1].tolist()) == w, c.name


def test_refusals():
    """k outside 2..13 and a piece bound above 2048 are refused by the C entry point before any launch (the count words keep
    their sentinel); the Python wrapper refuses a 2049-base piece."""
    import torch
    from svision_amd import _lib, kernels
    lib = _lib.load()
    x, y = kernels.pack_bases("ACGT" * 30), kernels.pack_bases("ACGT" * 60)
    desc = np.zeros(1, kernels.HASH_JOB_DTYPE)
    cap = 4 * len(y) + 64
    desc[0] = (0, len(x), len(x), len(y), 0, 2048, cap, 0)
    d_bases = torch.from_numpy(np.concatenate([x, y, np.zeros(16, np.uint8)])).to(DEV)
    d_jobs = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    d_table = torch.zeros(2048 * 2, dtype=torch.int64, device=DEV)
    d_hits = torch.zeros(2 * cap * 4, dtype=torch.int32, device=DEV)
    d_counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)

    def call(k, max_x):
        rc = lib.svx_hash_seeds(d_bases.data_ptr(), d_jobs.data_ptr(), 1, d_table.data_ptr(), d_hits.data_ptr(), d_counts.data_ptr(),
                                k, 50, max_x, kernels._stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        return rc

    for k, max_x in ((1, 2048), (14, 2048), (0, 2048), (10, 2049)):
        assert call(k, max_x) == _lib.SVX_EINVAL, (k, max_x)
        assert d_counts.tolist() == [-7, -7]
    assert call(10, 2048) == _lib.SVX_OK and d_counts.tolist() == [0, 0]          # the same arguments, accepted: it launches
    assert call(13, 2048) == _lib.SVX_OK and call(2, 2048) == _lib.SVX_OK
    long_piece = hc.by_name()[hc.TOO_LONG]
    with pytest.raises(_lib.SvxError):
        kernels.hash_seeds([(kernels.pack_bases(long_piece.seq), kernels.pack_bases(long_piece.ref))], 10, 50, DEV)


def test_collection_with_other_hash_options_device_equals_host():
    """detect_window --hash with k_size = 8, min_accept = 30, max_hash_len = 3000 on hash_collect.bam, device scan in both
    runs: the device seed kernel and the host aligner (rh.DEVICE = None) give the same signatures and TSV.  The yardstick is
    the host path (no reference golden at these options).
    Counted on the CPU under these options: 51 pieces reach the re-aligner, the longest has 771 bases (windows up to 7,771
    bases) -- none is longer than 1000 and none longer than 2048, so max_hash_len = 3000 lets no longer piece in on this
    sample; the options still change the result (52 signatures with helper segments against 53 at the defaults)."""
    from svision_amd import kernels
    from svision_amd.collection.output_clusters import collect_pair_lines
    from svision_amd.collection.run_collection import detect_window
    from svision_amd.io import bam
    from svision_amd.sample import Sample
    from svision_amd.segmentplot import run_hash_lineplot as rh
    fasta = helpers.load_golden_fasta("hash_collect.fa.gz")
    calls, params = [], set()
    orig, saved = kernels.hash_seeds, rh.DEVICE

    def spy(jobs, k, window, device):
        calls.append(len(jobs))
        params.add((k, window))
        return orig(jobs, k, window, device)

    results = []
    kernels.hash_seeds = spy
    try:
        for on_device in (True, False):
            table = bam.read_bam(os.path.join(helpers.GOLDEN, "hash_collect.bam"), with_seq=True)
            sample = Sample.from_table(table, fasta, 50, device=DEV)
            assert rh.DEVICE is not None
            if not on_device:
                rh.DEVICE = None
            before = sum(calls)
            opts = helpers.default_options(min_support=3, hash=True, k_size=8, min_accept=30, max_hash_len=3000)
            sigs, clusters = detect_window(opts, sample, "chrH", 0, 160_000)
            assert (sum(calls) - before > 20) == on_device               # the device kernel really ran / really did not
            results.append(([[s.type, s.tstart, s.tend, s.qname, s.bkps, s.mechanism,
                              [[a.q_start, a.q_end, a.ref_start, a.ref_end, bool(a.is_reverse)] for a in s.sorted_aligns]] for s in sigs],
                            "".join(p.text() for p in collect_pair_lines(clusters, opts))))
    finally:
        kernels.hash_seeds = orig
        rh.DEVICE = saved
    assert params == {(8, 30)}
    assert results[0][0] == results[1][0]
    assert results[0][1] == results[1][1]
    assert sum(1 for d in results[0][0] if len(d[6]) > 2) > 40 and results[0][1].count("\n") > 10
    with open(os.path.join(helpers.GOLDEN, "hash_collect.expected.json")) as f:
        assert results[0][0] != [w for w in json.load(f)["windows"] if w["hash"]][0]["signatures"]     # the options matter
