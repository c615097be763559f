"""--hash pieces of more than 2,048 bases without a device: the catalogue of tests/hashcases_long.py against the reference's
answers (tests/golden/hash_long.expected.json.gz, recorded by tests/golden/make_hash_long_fixture.py), what the catalogue must
hold for the tiled kernel's GPU tests (tests/test_gpu_hash_long.py), the two exports, and the routing switch
run_hash_lineplot.MAX_PIECE."""
import collections
import os
import re

import numpy as np

from svision_amd.segmentplot import run_hash_lineplot as rh
from tests import hashcases as hc
from tests import hashcases_long as hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_catalogue_is_the_one_the_reference_saw():
    want = hl.load_expected()
    cases = hl.all_cases()
    assert [c.name for c in cases] == list(want)
    for c in cases:
        w = want[c.name]
        assert (c.k, c.window, hc.digest(c)) == (w["k"], w["window"], w["crc"]), c.name
    assert want[hc.TOO_LONG]["segs"] == hc.load_expected()[hc.TOO_LONG]["segs"]      # the one-tile case: already in the other fixture
    assert all(len(c.seq) > hc.MAX_X for c in cases)
    assert [c.name for c in cases if not hl.device_eligible(c)] == [hl.TOO_LONG]


def test_host_aligner_and_replay_match_reference():
    """The host aligner's raw lists, replayed through the order-dependent host steps as the device's lists are, give the
    reference's final segments on every case (so the raw lists are a sound yardstick for the kernel); so does the host path."""
    want = hl.load_expected()
    for c in hl.all_cases():
        hits_a, hits_b = hc.raw_hit_lists_of(c)
        segs = rh._replay(np.asarray(hits_a, np.int32).reshape(-1, 4), np.asarray(hits_b, np.int32).reshape(-1, 4), len(c.seq), len(c.ref),
                          c.k, c.window)
        assert hc.fmt(segs) == want[c.name]["segs"], c.name
    for name in (hl.ONE_Y, hl.ALPHABET):
        c = hl.by_name()[name]
        assert hc.fmt(rh._hashplot_host(c.ref, c.seq, c.k, c.window)) == want[name]["segs"], name
    assert sum(bool(w["segs"]) for w in want.values()) >= 11


def test_catalogue_reaches_the_tile_edges():
    """On the host aligner's raw lists: what each case is there for."""
    cases = hl.by_name()
    assert hl.entries(cases[hc.TOO_LONG]) == 4076
    for k, _w in hl.EDGE_PARAMS:
        assert len(cases["l/edge4096/k%dw%d" % (k, _w)].seq) == 2048 + k + 1 and len(cases["l/edge4098/k%dw%d" % (k, _w)].seq) == 2048 + k + 2
    for name, last in (("l/edge4096/k2w2", 4095), ("l/edge4098/k2w2", 4097)):
        c = cases[name]
        nx = len(c.seq) - 3
        _a, hits_b = hc.raw_hit_lists_of(c)
        order = [h[1] if h[3] else nx + h[1] for h in hits_b if h[0] == 0]       # the entries "AC" (y position 0) hits, in list order
        assert order == sorted(order) and order[-1] == last and 4095 in order and nx - 1 in order and 0 in order, (name, order)
        assert len(hits_b) < 4 * len(c.ref) + 64
    c = cases[hl.STRAND]
    assert hl.entries(c) // 2 < hl.TILE < hl.entries(c) and {h[3] for h in hc.raw_hit_lists_of(c)[1]} == {0, 1}      # both strands in tile 0
    # one y position with hits in three tiles, forward ones in tiles 0 and 1, reverse-strand ones in tiles 1 and 2
    c = cases[hl.ONE_Y]
    _a, hits_b = hc.raw_hit_lists_of(c)
    y, n = collections.Counter(h[0] for h in hits_b).most_common(1)[0]
    assert n >= 4 and y == 300
    assert [(bool(h[3]), hl.tile_of(c, h[1], h[3])) for h in hits_b if h[0] == y] == [(True, 0), (True, 1), (False, 1), (False, 2)]
    c = cases[hl.CHUNK_EDGE]
    _a, hits_b = hc.raw_hit_lists_of(c)
    assert [h[0] for h in hits_b] == [255, 256, 257] and {hl.tile_of(c, h[1], h[3]) for h in hits_b} == {1}
    c = cases[hl.OVERFLOW]
    hits_a, hits_b = hc.raw_hit_lists_of(c)
    assert len(hits_b) > 2900 and 4 * len(c.ref) + 64 == 88
    c = cases[hl.ALPHABET]
    assert len(c.seq) == 4000 and set(c.ref + c.seq) == set("ACGTNacgtnRYKMS") and "N" * 40 in c.seq
    assert len(hc.raw_hit_lists_of(c)[1]) >= 3
    c = cases[hl.SIX_TILES]
    assert (len(c.seq), len(c.ref), (hl.entries(c) + hl.TILE - 1) // hl.TILE) == (12000, 20000, 6)
    assert len({hl.tile_of(c, h[1], h[3]) for h in hc.raw_hit_lists_of(c)[1]}) == 6
    assert (len(cases[hl.LONGEST].seq), len(cases[hl.LONGEST].ref)) == (65536, 70000) and len(cases[hl.TOO_LONG].seq) == 65537


def test_exports_are_declared_and_sized():
    from svision_amd import _lib, kernels
    header = open(os.path.join(ROOT, "include", "svx.h")).read()
    for name in ("svx_hash_seeds_long", "svx_hash_seeds_long_ws_bytes"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", " ", header, flags=re.S)), name
    lib = _lib.load()
    assert lib.svx_version() == 420
    assert lib.svx_hash_seeds_long is not None
    for x_len, y_len in ((0, 0), (2049, 3000), (2049, 3001), (6000, 9000), (65536, 70000), (65536, (1 << 26) - 1), (1, 1), (3, 5)):
        assert lib.svx_hash_seeds_long_ws_bytes(x_len, y_len) == (16 * x_len + 4 * y_len + 15) // 16 * 16, (x_len, y_len)
    assert kernels.HASH_LONG_MAX_X == hl.LONG_MAX_X == 65536 and kernels.HASH_MAX_X == 2048


def _remote_request(monkeypatch, max_piece):
    """hashplot_unmapped_batch in a helper's place (no device, a REMOTE stand-in that answers from the host aligner's raw
    lists): -> (the piece lengths in the request, the batch's results)."""
    from tests.test_hash_batch_cpu import _answer
    seen = []

    def remote(bases, desc, k, min_accept):
        seen.extend(desc[:, 1].tolist())
        return _answer(("hash", 0, k, min_accept, bases, desc))[2:]

    monkeypatch.setattr(rh, "REMOTE", remote)
    monkeypatch.setattr(rh, "MAX_PIECE", max_piece)
    cases = [hc.by_name()[hc.ONE_Y], hl.by_name()[hl.STRAND], hc.by_name()[hc.CHUNK_EDGE]]
    assert [len(c.seq) for c in cases][1] == 3000
    got = rh.hashplot_unmapped_batch([(c.ref, c.seq) for c in cases], 10, 50, None)
    return cases, seen, got


def test_max_piece_lets_a_long_job_into_the_request(monkeypatch):
    from svision_amd import kernels
    cases, seen, got = _remote_request(monkeypatch, kernels.HASH_LONG_MAX_X)
    assert seen == [len(c.seq) for c in cases] and 3000 in seen
    assert hc.fmt(got[1]) == hl.load_expected()[hl.STRAND]["segs"]
    assert [hc.fmt(got[0]), hc.fmt(got[2])] == [hc.load_expected()[n]["segs"] for n in (hc.ONE_Y, hc.CHUNK_EDGE)]
    # a piece above the bound stays out of it
    too_long = hl.by_name()[hl.TOO_LONG]
    del seen[:]
    assert rh.hashplot_unmapped_batch([(too_long.ref, too_long.seq)], 10, 50, None) == [None] and seen == []


def test_without_max_piece_a_long_job_stays_out(monkeypatch):
    assert rh.MAX_PIECE is None                                          # the module's default
    cases, seen, got = _remote_request(monkeypatch, None)
    assert seen == [len(cases[0].seq), len(cases[2].seq)] and got[1] is None and got[0] is not None and got[2] is not None
