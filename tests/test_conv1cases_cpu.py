"""CPU test of tests/conv1cases.py: with the Python oracle (oracle/encode_ref.py), every crafted image contains what its name claims,
and the restatements the GPU tests compare with agree with the project's other restatements of the same operations."""
import numpy as np
import pytest

from oracle import alexnet_ref, encode_ref
from tests import cnncases
from tests import conv1cases as k1
from tests.test_image_golden import touched_from_pixels


@pytest.fixture(scope="module")
def masks():
    return k1.oracle_masks(None)


@pytest.fixture(scope="module")
def census(masks):
    return k1.window_census(masks)


def test_the_table_holds_the_four_groups(masks):
    t = k1.cases()
    assert masks.shape == (len(t), 227, 227, 3)
    assert [len(k1.group_ids(g)) for g in "abc"] == [6 * 227, len(k1.PAIR_COLS) * len(k1.PAIR_GAPS), 5]
    e = k1.empty_ids()
    assert e[0] == 0 and e[-1] == len(t) - 1 and len(e) == 3 and 0 < e[1] < len(t) - 1           # first, inside and last
    assert tuple(t[-2].rec) == encode_ref.PAD_RECORD
    assert all(c.rec[10] == c.rec[11] for c in t) and {c.rec[10] for c in t} == {1, 2, 227}     # ratio 1 everywhere
    ids = k1.mixed_ids()
    assert 35 <= len(ids) <= 45 and ids[0] == e[0] and ids[-1] == e[2] and e[1] in ids
    assert {t[i].group for i in ids} == {"a", "b", "c", "d"}


def test_pixel_counts_per_channel(masks):
    t = k1.cases()
    got = masks.sum((1, 2))
    bad = [(c.name, got[i].tolist()) for i, c in enumerate(t) if tuple(got[i]) != c.counts]
    assert not bad, bad[:5]
    assert tuple(got[k1.group_ids("c")[0]]) == (453, 452, 227)                                   # the two diagonals
    assert not masks[k1.empty_ids()].any()


def test_group_a_puts_the_pixel_where_its_name_says(masks):
    t = k1.cases()
    fwd = rev = twice = short = 0
    for i in k1.group_ids("a"):
        r, _r1, c, _c1, f = t[i].rec[:5]
        assert masks[i, r, c, 0] and masks[i, :, :, 0].sum() == 1
        assert masks[i, r, c, 2] == (f == 0) and not masks[i, :, :, 1].any()
        fwd += f
        rev += 1 - f
        twice += t[i].rec[5:10] == t[i].rec[:5]
        short += t[i].rec[10] == 1
    n = len(k1.group_ids("a"))
    assert fwd == rev == n // 2 and abs(2 * twice - n) <= 2 and abs(2 * short - n) <= 4


def test_group_a_reaches_every_window_offset_and_word_boundary(masks):
    """window_mask(row, c0) reads 11 bits from bit offset c0.  Every c0 the kernel forms is a multiple of 4 (conv stride 4): 0 .. 216, so
    sh = c0 & 31 takes the values 0, 4 .. 28 -- not every value below 32 -- and the second word is fetched at sh = 24 and 28.  Each of
    the 55 offsets must occur with a set pixel at bit 0 and at bit 10 of the window, on each probe row (planes) and, for the rows, on
    each probe column (rowany is indexed by column too, the conv rows by 4 * oy + ky).  The last window starts at bit 216 of word 6:
    its second word is word 7, so the spare word behind colmask is never read."""
    have = {tuple(k1.cases()[i].rec[0:3:2]) for i in k1.group_ids("a")}                          # (row, col)
    offsets = range(0, 4 * k1.CONV1, 4)
    assert {c0 & 31 for c0 in offsets} == set(range(0, 32, 4))
    second_word = [c0 for c0 in offsets if (c0 & 31) > 21]
    assert {c0 & 31 for c0 in second_word} == {24, 28} and all((c0 + 10) >> 5 == (c0 >> 5) + 1 for c0 in second_word)
    assert max(offsets) == 216 and (216 >> 5) + 1 == 7
    for line in k1.PROBE_LINES:
        for c0 in offsets:
            assert (line, c0) in have and (line, c0 + 10) in have
            assert (c0, line) in have and (c0 + 10, line) in have
    assert max(c0 + 10 for c0 in offsets) == 226
    ne = k1.window_nonempty(masks[k1.group_ids("a")])
    assert ne[:, 0, 0].any() and ne[:, 0, 54].any() and ne[:, 54, 0].any() and ne[:, 54, 54].any()      # the first and the last window


def test_group_b_sets_channel_1_at_both_pixels_and_channel_2_at_its_own(masks):
    t = k1.cases()
    same_window = next_window = other_strip = 0
    for i in k1.group_ids("b"):
        r1, c = t[i].rec[0], t[i].rec[2]
        r2, fwd2 = t[i].rec[5], t[i].rec[9]
        assert t[i].rec[7] == c and r2 - r1 in k1.PAIR_GAPS
        want = np.zeros((227, 227), bool)
        want[[r1, r2], c] = True
        assert np.array_equal(masks[i, :, :, 0], want) and np.array_equal(masks[i, :, :, 1], want)
        want[r1, c] = False
        assert np.array_equal(masks[i, :, :, 2], want if fwd2 == 0 else np.zeros_like(want))
        same_window += r2 - r1 < 11
        next_window += 11 <= r2 - r1 < 19
        other_strip += r2 - r1 > 18                       # no pooled row (19 image rows) sees both: the strip that draws one needs colmask for the other
    assert same_window and next_window and other_strip
    assert {t[i].rec[2] for i in k1.group_ids("b")} == set(k1.PAIR_COLS)


def test_group_c_has_pooled_pixels_with_nine_eight_and_fewer_windows(masks, census):
    c = k1.group_ids("c")
    two = census[c[0]]
    assert [(two == v).sum() for v in (9, 8, 6)] == [53, 4, 96]
    for i in c[:4]:
        assert (census[i] == 9).any() and ((census[i] > 0) & (census[i] < 8)).any(), k1.cases()[i].name
    assert (census[c[3]] == 8).any()
    assert not census[k1.empty_ids()].any()


def test_touched_pixels_are_the_pooled_receptive_fields(masks, census):
    t = k1.touched_pixels(masks)
    assert np.array_equal(t, census > 0)
    for i in k1.mixed_ids():
        pix = [np.flatnonzero(masks[i, :, :, ch].reshape(-1)) for ch in range(3)]
        assert np.array_equal(k1.to_words(t[i]), touched_from_pixels(pix)), k1.cases()[i].name
    w = k1.to_words(t)
    assert w.dtype == np.uint32 and not (w >> 27).any() and np.array_equal(k1.from_words(w), t)
    pad = t[len(k1.cases()) - 2]
    assert pad[0, 0] and pad.sum() == 1 and not t[0].any()


def test_weight_set_b_tells_the_empty_window_floor_from_zero(masks, census):
    """In fp64, channels 0 .. 47 of set B: a pooled pixel of the two-diagonal image with nine non-empty windows lies far below
    relu(base) = 50 (a kernel that starts it at relu(base) is wrong by that much), one with eight at exactly 50 (a kernel that starts
    it at 0 is wrong there)."""
    w1, base = k1.weights_b()
    assert (w1[..., :48] < 0).all() and (w1[..., 48:] > 0).all() and (base[:48] == 50).all() and (base[48:] == -50).all()
    i = k1.group_ids("c")[0]
    pooled, bound = k1.conv1_ref64(masks[i:i + 1], w1, base)
    nine, eight = census[i] == 9, census[i] == 8
    assert bound.max() < 0.05
    assert (pooled[0][nine][:, :48] < 50 - 5).all()
    assert (pooled[0][eight][:, :48] == 50).all() and (pooled[0][census[i] == 0][:, :48] == 50).all()
    assert (pooled[0][census[i] == 0][:, 48:] == 0).all() and (pooled[0][nine][:, 48:] > 1).any()
    wa, ba = k1.weights_a()
    pa, _b = k1.conv1_ref64(masks[i:i + 1], wa, ba)
    floor = np.maximum(ba.astype(np.float64), 0)
    assert (pa[0][nine] >= floor).mean() > 0.9        # with random weights some window nearly always exceeds relu(base): either start passes


def test_conv1_restatement_is_the_oracle_s_layer_without_the_mean(masks):
    """base = bias - sum(mean * w) turns the restatement into the oracle's conv1 of the mean-subtracted image (float32 there)."""
    ids = k1.group_ids("c")[:2] + k1.group_ids("b")[:2] + [0]
    w1, _base = k1.weights_a()
    bias = np.linspace(-1, 1, 96).astype(np.float32)
    mean = np.asarray(encode_ref.MEAN, np.float64)
    base = (bias - (w1.astype(np.float64) * mean[None, None, :, None]).sum((0, 1, 2))).astype(np.float32)
    pooled, bound = k1.conv1_ref64(masks[ids], w1, base)
    x = encode_ref.encode_records(k1.records()[ids])
    a = alexnet_ref._conv_layer(x, w1, bias, 4, "VALID", 1)
    want = alexnet_ref._max_pool_3x3s2_valid(a)
    assert pooled.shape == want.shape == (len(ids), 27, 27, 96)
    assert np.abs(pooled - want).max() < 1e-3 and (bound > 0).all()
    for _name, radius, alpha, beta, k in k1.lrn_params():
        ref = alexnet_ref._lrn(np.ascontiguousarray(pooled), radius=radius, alpha=alpha, beta=beta, bias=k)
        assert np.array_equal(k1.lrn64(pooled, radius, alpha, beta, k).astype(np.float32), ref)
    assert len(k1.lrn_params()) == len(cnncases.POOL_PARAMS) + 1 and max(p[1] for p in k1.lrn_params()) == 96


def test_active_set_restatement_and_its_touched_sets():
    single = k1.single_bit_touched()
    assert single.shape == (729, 27, 27) and (single.sum((1, 2)) == 1).all() and single.any(0).all()
    assert max(k1.SINGLE_CUTS) == 729 and {255, 256, 257} < set(k1.SINGLE_CUTS)
    a2, a3, a4, a5 = k1.active_masks(single)
    assert a2[0].sum() == 9 and a2[14 * 27 + 13].sum() == 25 and a3[0].sum() == 9 and a5[0].sum() == 25      # corner: 3x3, centre: 5x5
    lists, counts, rows2, add = k1.expected_active_sets(single, live=3)
    assert [len(v) for v in lists] == [3 * 729, 3 * 169, 3 * 169, 3 * 169] and rows2.shape == (3, 27) and add[4] == 729
    assert counts[0] == 9 + 12 + 15 and lists[0][:counts[0]].tolist() == sorted(lists[0][:counts[0]].tolist())
    assert sorted(lists[1].tolist()) == list(range(3 * 169))
    lists0, counts0, rows0, add0 = k1.expected_active_sets(single, live=0)
    assert counts0 == [0] * 4 and add0 == [0, 0, 0, 0, 729] and rows0.shape == (0, 27) and all(v.size == 0 for v in lists0)
    ef = k1.empty_and_full_touched()
    _l, counts, _r, add = k1.expected_active_sets(ef)
    assert counts == [3 * 729, 3 * 169, 3 * 169, 3 * 169] and add == [3 * 729, 3 * 169, 3 * 169, 3 * 169, 5]


def test_the_threshold_sets_sit_on_the_dense_rule_and_one_pixel_below():
    at, total_at = k1.threshold_touched(0)
    below, total_below = k1.threshold_touched(1)
    every = at.shape[0] * 729
    assert total_below == total_at - 1
    assert total_at * 100 >= every * k1.DENSE_PCT > (total_at - 1) * 100
    for t, total in ((at, total_at), (below, total_below)):
        assert (t.sum((1, 2)) == 729).sum() == t.shape[0] - 1                  # full images and one partial one
        _l, counts, _r, add = k1.expected_active_sets(t)
        assert counts[0] == total
        assert add[0] == (every if t is at else total)
    assert k1.executed(97, 100) == 100 and k1.executed(96, 100) == 96 and k1.executed(0, 0) == 0
    assert k1.DENSE_PCT == cnncases.DENSE_PCT
    assert k1.live_values(40) == [0, 1, 39, 40, 45] and k1.live_values(1) == [0, 1, 6]
