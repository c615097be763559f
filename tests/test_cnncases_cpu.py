"""CPU test of tests/cnncases.py: the catalogue reaches the code paths its names promise, at 1,024 SIMDs (a whole MI355X) and at 128 (a
partitioned one), and the one planning rule the library exports agrees with its restatement."""
import numpy as np
import pytest

from tests import cnncases as cc

SIMDS = [1024, 128]


@pytest.mark.parametrize("n_simd", SIMDS)
def test_shape_1_is_reached_dense_and_listed_at_both_kernel_sizes(n_simd):
    seen = set()
    for name, (cin, cout, hw, ksize, groups) in cc.SHAPE1_LAYERS.items():
        n1 = cc.smallest_n_for_shape(1, cin, cout, hw, groups, n_simd, cc.N_SHAPES)
        assert n1 is not None and 1 < n1 <= 64, name
        assert cc.conv_pick_shape(n1 * hw * hw, cout // groups, groups, n_simd) == 1
        assert cc.conv_pick_shape((n1 - 1) * hw * hw, cout // groups, groups, n_simd) == 0       # the other side of the switch
        seen.add((ksize, "dense"))
        plan = cc.list_shape1_plan(cout, hw, groups, n_simd)
        assert plan is not None, name
        n, count1, count0 = plan
        assert n <= 64 and count0 == count1 - 1
        assert cc.conv_pick_shape(count1, cout // groups, groups, n_simd, cc.LIST_SHAPES) == 1
        assert cc.conv_pick_shape(count0, cout // groups, groups, n_simd, cc.LIST_SHAPES) == 0
        assert cc.list_is_followed(count1, n * hw * hw) and cc.list_is_followed(count0, n * hw * hw)
        assert cc.list_is_followed(count1 + cc.LIST_MARGIN, n * hw * hw)                         # comfortably
        seen.add((ksize, "list"))
    assert seen == {(3, "dense"), (3, "list"), (5, "dense"), (5, "list")}


def test_the_searches_give_the_quoted_sizes_on_a_whole_device():
    assert cc.smallest_n_for_shape(1, 96, 256, 27, 2, 1024, cc.N_SHAPES) == 12
    assert cc.smallest_n_for_shape(1, 256, 384, 13, 1, 1024, cc.N_SHAPES) == 33
    assert cc.smallest_count_for_shape(1, 256, 2, 1024, 64 * 729) == 8193
    assert cc.smallest_count_for_shape(1, 384, 1, 1024, 64 * 169) == 5441
    assert cc.smallest_n_for_shape(2, 256, 384, 13, 1, 1024, cc.N_SHAPES) is None


def test_the_tail_cases_leave_one_and_two_octets():
    left = [cc.conv_q(5, cin // groups) % 3 for _name, _n, cin, _cout, _h, _w, groups in cc.CONV_TAIL_CASES]
    assert set(left) == {1, 2} and 0 not in left
    assert [cin // groups for _name, _n, cin, _cout, _h, _w, groups in cc.CONV_TAIL_CASES] == [16, 32, 64]
    for cin_g in range(16, 513, 16):                          # every 3x3 layer the entry point accepts has an empty tail
        assert cc.conv_q(3, cin_g) % 3 == 0
    for _name, _n, cin, cout, h, w, groups in cc.CONV_TAIL_CASES:
        assert h != w and (cin // groups) % 16 == 0 and (cout // groups) % 64 == 0


@pytest.mark.parametrize("n_simd", SIMDS)
def test_the_grid_sweep_reaches_the_edges_of_the_work_distribution(n_simd):
    ms = [n * h * w for _name, n, h, w in cc.GRID_IMAGES]
    assert ms == [1, 31, 32, 33, 95, 96, 97, 255, 256, 257, 1001]
    assert [(h, w) for _name, _n, h, w in cc.GRID_IMAGES if h == w and h > 1] == [(16, 16)]       # all others: non-square or degenerate
    odd = small = few = few8 = 0
    for _cname, cout, groups in cc.GRID_CHANNELS:
        assert (cout // groups) % 64 == 0
        for M in ms:
            shape = cc.conv_pick_shape(M, cout // groups, groups, n_simd)
            assert shape in (0, 1) and (shape == 0 or n_simd < 1024)     # on a whole device the sweep runs shape 0 throughout
            g = cc.conv_grid(M, cout // groups, groups, shape)
            assert cc.conv_grid_covers(M, cout // groups, groups, shape)
            odd += g["ny"] > 1 and g["ny"] % 2 == 1
            small += M < 32
            few += g["halves"] == 2 and g["m_tiles"] < 4      # fewer pixel tiles than the four pixel ranges
            few8 += g["halves"] == 1 and g["m_tiles"] < 8     # ... than the eight
    assert odd and small and few and few8
    assert {cc.conv_grid(32, cout // groups, groups, 0)["ny"] for _c, cout, groups in cc.GRID_CHANNELS} == {1, 3, 5, 2, 4, 6}


def test_the_restated_distribution_gives_every_tile_one_wave():
    """conv_grid_covers on many sizes, both list shapes: no tile without a wave, none with two."""
    rng = np.random.default_rng(7)
    for M in list(range(1, 200)) + [int(v) for v in rng.integers(200, 60_000, 60)]:
        for cout_g, groups in ((64, 1), (192, 1), (128, 2), (384, 1), (192, 2)):
            for shape in range(cc.LIST_SHAPES):
                assert cc.conv_grid_covers(M, cout_g, groups, shape), (M, cout_g, groups, shape)


def test_list_cases_sit_on_their_thresholds():
    n, _cin, _cout, h, w, _k, _g = cc.LIST_EDGE_LAYER
    mall = n * h * w
    assert mall == 338
    for c in cc.LIST_EDGE_COUNTS + [mall - r for r in cc.LIST_FILL_REMAINDERS]:
        assert cc.list_is_followed(c, mall)
    assert {c for c in cc.LIST_EDGE_COUNTS} >= {31, 32, 33, 95, 96, 97}
    assert cc.FILL_PIX in cc.LIST_FILL_REMAINDERS and cc.FILL_PIX - 1 in cc.LIST_FILL_REMAINDERS and cc.FILL_PIX + 1 in cc.LIST_FILL_REMAINDERS
    n, _cin, _cout, h, w, _k, _g = cc.DENSE_RULE_LAYER
    assert n * h * w == 100
    assert [cc.list_is_followed(c, 100) for _name, c, _f in cc.DENSE_RULE_COUNTS] == [f for _name, _c, f in cc.DENSE_RULE_COUNTS] == [True, False, False]
    n = cc.LIST_LIVE_LAYER[0]
    assert min(cc.LIST_LIVE_VALUES) == 1 and n in cc.LIST_LIVE_VALUES and n - 1 in cc.LIST_LIVE_VALUES and max(cc.LIST_LIVE_VALUES) > n


def test_pixel_list_is_the_kernel_s_permutation():
    lst = cc.pixel_list([7, 2, 9], 12)
    assert lst.dtype == np.int32 and lst.tolist() == [2, 7, 9, 0, 1, 3, 4, 5, 6, 8, 10, 11]
    assert cc.pixel_list([], 3).tolist() == [0, 1, 2] and cc.pixel_list(range(3), 3).tolist() == [0, 1, 2]


def test_fc_cases_cover_every_instantiation_and_every_tail():
    for name, m, n in cc.FC_TAIL_MN:
        assert "<%d,%d>" % cc.fc_instantiation(m, n) == name
        left = []
        for k in cc.FC_TAIL_K:
            q = cc.fc_q_lengths(m, n, k)
            assert len(q) == 1 and q[0] == k // 8              # one split: the whole of k
            left.append(q[0] % cc.FC_RING)
        assert sorted(left) == [0, 1, 2, 3, 4, 5], name
    inst = {}
    for name, m, n, k in cc.FC_ROW_TILE_CASES:
        inst.setdefault(cc.fc_instantiation(m, n), []).append(cc.fc_row_tiles(m))
        assert sum(cc.fc_q_lengths(m, n, k)) == k // 8 and min(cc.fc_q_lengths(m, n, k)) >= cc.FC_MIN_OCTETS
    assert max(inst[(1, 2)]) == 3 and 2 in inst[(1, 2)]       # <1,2> with several row tiles: m > 64 and n % 64 != 0
    assert set(inst) == {(1, 1), (1, 2), (2, 2)}
    assert {cc.fc_instantiation(cc.FC_LIVE_M, n) for n in cc.FC_LIVE_N} == {(2, 2), (1, 2)}
    assert {1, 32, 33, 64, 65, cc.FC_LIVE_M, cc.FC_LIVE_M + 7} == set(cc.FC_LIVE_VALUES)


def test_fc_splits_is_the_library_s():
    """svx_fc_ws_bytes(m, n, k) == splits * m * n * 4: the restated split rule is the one the entry point sizes its scratch by."""
    from svision_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(11)
    cases = cc.fc_cases() + [(64, 4096, 9216), (64, 4096, 4096), (256, 4096, 4096), (1, 32, 192)]
    for _ in range(400):
        cases.append((int(rng.integers(1, 400)), 32 * int(rng.integers(1, 160)), 8 * int(rng.integers(24, 1400))))
    for m, n, k in cases:
        assert lib.svx_fc_ws_bytes(m, n, k) == cc.fc_splits(m, n, k) * m * n * 4, (m, n, k)
    assert len({cc.fc_splits(m, n, k) for m, n, k in cases}) > 20


def _pick_many(M, cout_g, groups, n_simd, n_shapes):
    """conv_pick_shape on an array of pixel counts (argmin takes the first minimum: ties go to the earlier shape)."""
    units = np.full((n_shapes, M.size), np.iinfo(np.int64).max)
    for s in range(n_shapes):
        if cout_g % (32 * cc.SHAPE_NA[s]) == 0:
            tiles = -(-M // (32 * cc.SHAPE_NB[s])) * groups * (cout_g // (32 * cc.SHAPE_NA[s]))
            units[s] = -(-tiles // n_simd) * cc.SHAPE_NA[s] * cc.SHAPE_NB[s]
    return units.argmin(0)


def test_dense_shapes_2_to_4_are_never_picked():
    """The GPU cases aim at shapes 0 and 1 only because the rule never picks another one (tests/cnncases.py has the argument).  If
    this fails the rule has changed: extend tests/test_gpu_cnn_tiles.py to the shapes that can now run."""
    M = np.arange(1, 1 << 18, dtype=np.int64)
    rng = np.random.default_rng(3)
    picked = set()
    for n_simd in (1024, 512, 128):
        for cout_g in range(64, 513, 64):
            for groups in (1, 2):
                got = _pick_many(M, cout_g, groups, n_simd, cc.N_SHAPES)
                picked |= set(np.unique(got).tolist())
                for m in rng.integers(1, M.size, 8):          # the array form is the scalar rule
                    assert got[m - 1] == cc.conv_pick_shape(int(m), cout_g, groups, n_simd)
                assert np.array_equal(np.minimum(got, 1), _pick_many(M, cout_g, groups, n_simd, cc.LIST_SHAPES))
    assert picked == {0, 1}
