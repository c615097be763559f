"""The host --hash aligner (svision_amd/segmentplot/hash_aligner.py) vs the reference's hashplot_unmapped beyond k = 10,
window = 50: the cases of tests/hashcases.py, the reference's answers recorded by tests/golden/make_hash_params_fixture.py.
Also proves that the catalogue holds what the device tests (tests/test_gpu_hash_seeds.py) rely on."""
import collections

from svision_amd.segmentplot import run_hash_lineplot as rh
from tests import hashcases as hc


def test_catalogue_is_the_one_the_reference_saw():
    want = hc.load_expected()
    cases = hc.all_cases()
    assert [c.name for c in cases] == list(want)
    for c in cases:
        w = want[c.name]
        assert (c.k, c.window, hc.digest(c)) == (w["k"], w["window"], w["crc"]), c.name
    assert sum(1 for c in cases if c.k == 14) == 3
    assert {(c.k, c.window) for c in cases if c.name.startswith("a/")} == set(hc.SWEEP)
    assert {(c.k, c.window) for c in cases if c.name.startswith("b/")} == set(hc.TINY)
    assert sorted(len(c.seq) for c in cases if c.name.startswith("c/")) == sorted(hc.FULL_LENS * 3 + [hc.MAX_X + 1])
    wide = [c for c in cases if c.name.startswith("a/") and set(c.ref) - set("ACGT")]
    assert len(wide) == len(hc.SWEEP) * hc.SWEEP_PER_PARAM // 3
    assert set("".join(c.ref + c.seq for c in wide)) == set("ACGTNacgtnRYKMS")


def test_host_aligner_matches_reference_at_other_parameters():
    want = hc.load_expected()
    cases = hc.all_cases()
    got = {}
    for c in cases:
        got[c.name] = hc.fmt(rh._hashplot_host(c.ref, c.seq, c.k, c.window))
        assert got[c.name] == want[c.name]["segs"], c.name
    # the catalogue is not vacuous
    planted, found = collections.Counter(), collections.Counter()
    for c in cases:
        if hc.is_planted(c):
            planted[hc.sweep_group(c)] += 1
            found[hc.sweep_group(c)] += bool(got[c.name])
    assert len(planted) == len(hc.SWEEP)
    for g in planted:
        assert 3 * found[g] >= planted[g], (g, found[g], planted[g])
    for name in hc.ALL_AVOIDED:
        assert got[name] == []


def test_catalogue_reaches_the_kernel_edges():
    """On the host aligner's raw lists: the overflow case overflows, case d spreads over 256-chunks of y, case e has several
    hits at one y on both strands, the all-avoided cases have no seed, the full-table cases fill the table."""
    cases = hc.by_name()
    c = cases[hc.OVERFLOW]
    hits_a, hits_b = hc.raw_hit_lists_of(c)
    assert len(hits_a) == 1 and len(hits_b) == 1023 > 4 * len(c.ref) + 64 == 88
    for name in hc.ALL_AVOIDED:
        assert hc.raw_hit_lists_of(cases[name]) == ([], [])
    _a, hits_b = hc.raw_hit_lists_of(cases[hc.CHUNKS])
    chunks = collections.Counter(h[0] // 256 for h in hits_b)
    assert len(chunks) >= 4 and max(chunks.values()) >= 2
    assert {0, 1} == {h[3] for h in hits_b}
    _a, hits_b = hc.raw_hit_lists_of(cases[hc.CHUNK_EDGE])
    assert [h[0] for h in hits_b] == [255, 256, 257]
    _a, hits_b = hc.raw_hit_lists_of(cases[hc.ONE_Y])
    y, n = collections.Counter(h[0] for h in hits_b).most_common(1)[0]
    assert n >= 3 and {h[3] for h in hits_b if h[0] == y} == {0, 1}
    full = [c for c in cases.values() if c.name.startswith("c/") and c.k == 2]
    assert max(2 * (len(c.seq) - (c.k + 1)) for c in full) == 4090       # entries of the kernel's LDS table (4096)
    assert len(cases[hc.LARGE].ref) == 20000 and len(cases[hc.LARGE].seq) == 2000
