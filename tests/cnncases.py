"""The planning rules of the CNN matrix kernels, restated, and the shapes their tests share.

Everything here is plain Python and NumPy: no torch, no product import.  The first part RESTATES rules of the kernels --
``SHAPE_NA`` / ``SHAPE_NB``, ``conv_wave_tiles``, ``conv_pick_shape`` and the XCD distribution of ``conv_wave_tile`` from
svision_amd/csrc/svx_conv.hip, ``fc_na`` / ``fc_splits`` and the split bounds of ``fc_splitk_kernel`` from svision_amd/csrc/svx_fc.hip -- so
that a test can say, on the host, WHICH code path a shape takes on the device it runs on: which wave tile shape, how long the k loop's
tail is, how many row tiles and splits.  Nothing here computes an expected value.  If the kernels' rules drift away from these, the
comparisons of tests/test_gpu_cnn_tiles.py with fp64 still hold and only the targeting is lost; tests/test_cnncases_cpu.py pins the one
rule the library exports (the fc split count, through ``svx_fc_ws_bytes``) and checks what the catalogue claims about itself.

The second part is the catalogue: every entry starts with a name that says what it singles out.

Finding recorded for a later clean-up: the dense tile shapes 2, 3 and 4 (64 x 96, 64 x 64, 32 x 64) are never picked, for any pixel
count, channel count, group count and SIMD count.  ``conv_pick_shape`` minimises ceil(tiles / SIMDs) * NA * NB with ties to the earlier
shape, and with r = ceil(M / 32), ny = groups * cout_g / 64:
  * shape 3 (2 x 2): tiles0 = r * ny <= 2 * ceil(r / 2) * ny = 2 * tiles3, so ceil(tiles0 / S) * 2 <= ceil(tiles3 / S) * 4;
  * shape 4 (1 x 2): tiles4 = ceil(r / 2) * 2 * ny >= tiles0, so ceil(tiles0 / S) * 2 <= ceil(tiles4 / S) * 2;
  * shape 2 (2 x 3): tiles1 = 2 * tiles2, so ceil(tiles1 / S) * 3 <= ceil(tiles2 / S) * 6 (shape 1 is valid wherever shape 2 is).
Without an experiment build they cannot run, which is why no case below aims at them.
"""
import numpy as np

# ---- svx_conv.hip ----
N_SHAPES = 5
SHAPE_NA = (2, 1, 2, 2, 1)          # wave tile = 32 * NA channels x 32 * NB pixels
SHAPE_NB = (1, 3, 3, 2, 2)
LIST_SHAPES = 2                     # list mode picks among the first two, on the device
DENSE_PCT = 97                      # include/svx.h SVX_CONV_DENSE_PCT: a list this full is not followed
FILL_PIX = 128                      # pixels of one background-copy unit
WAVES = 4                           # waves per workgroup


def conv_wave_tiles(M, cout_g, groups, shape):
    return -(-M // (32 * SHAPE_NB[shape])) * groups * (cout_g // (32 * SHAPE_NA[shape]))


def conv_pick_shape(M, cout_g, groups, n_simd, n_shapes=N_SHAPES):
    """The shape whose busiest SIMD runs the fewest accumulator-units; ties go to the earlier shape."""
    best, best_units = -1, 0
    for s in range(n_shapes):
        if cout_g % (32 * SHAPE_NA[s]):
            continue
        tiles = conv_wave_tiles(M, cout_g, groups, s)
        units = -(-tiles // n_simd) * SHAPE_NA[s] * SHAPE_NB[s]
        if best < 0 or units < best_units:
            best, best_units = s, units
    return best


def conv_q(ksize, cin_g):
    """Octets of k the loop walks; the loop body takes three, the tail Q % 3."""
    return ksize * ksize * cin_g // 8


def conv_grid(M, cout_g, groups, shape):
    """The XCD distribution of conv_wave_tile: pixel tiles, channel tiles, channel halves (1 when the channel-tile count is odd),
    pixel tiles per pixel range, compute workgroups per XCD."""
    m_tiles = -(-M // (32 * SHAPE_NB[shape]))
    ny = groups * (cout_g // (32 * SHAPE_NA[shape]))
    halves = 1 if ny & 1 else 2
    mp = (m_tiles * halves + 7) // 8
    per_c = (mp * (ny // halves) + WAVES - 1) // WAVES
    return dict(m_tiles=m_tiles, ny=ny, halves=halves, ranges=8 // halves, mp=mp, per_c=per_c)


def conv_grid_covers(M, cout_g, groups, shape):
    """Does every (pixel tile, channel tile) get exactly one wave under the kernel's index arithmetic?  (host restatement)"""
    g = conv_grid(M, cout_g, groups, shape)
    n_half = g["ny"] // g["halves"]
    seen = {}
    for xcd in range(8):
        for wl in range(g["per_c"] * WAVES):
            if wl >= g["mp"] * n_half:
                continue
            mt = (xcd // g["halves"]) * g["mp"] + wl // n_half
            if mt >= g["m_tiles"]:
                continue
            key = (mt, (xcd % g["halves"]) * n_half + wl % n_half)
            seen[key] = seen.get(key, 0) + 1
    return len(seen) == g["m_tiles"] * g["ny"] and all(v == 1 for v in seen.values())


def list_is_followed(count, mall):
    """svx_conv2d_same computes the listed pixels only below DENSE_PCT percent, every pixel from there on."""
    return count * 100 < mall * DENSE_PCT


def smallest_n_for_shape(shape, cin, cout, hw, groups, n_simd, n_shapes=N_SHAPES, cap=64):
    """The smallest image count (hw x hw pixels each) for which the rule picks ``shape``, or None up to ``cap``.  (cin takes no part in
    the rule; it is here so that a layer's tuple can be passed whole.)"""
    for n in range(1, cap + 1):
        if conv_pick_shape(n * hw * hw, cout // groups, groups, n_simd, n_shapes) == shape:
            return n
    return None


def smallest_count_for_shape(shape, cout, groups, n_simd, limit, n_shapes=LIST_SHAPES):
    """The smallest listed-pixel count (1 .. limit) for which the device-side rule of list mode picks ``shape``, or None."""
    for count in range(1, limit + 1):
        if conv_pick_shape(count, cout // groups, groups, n_simd, n_shapes) == shape:
            return count
    return None


LIST_MARGIN = FILL_PIX              # "comfortably above": the switch count + one copy unit is still below DENSE_PCT percent


def list_shape1_plan(cout, hw, groups, n_simd, cap=64):
    """(n, count1, count0) for list mode: count1 the smallest count that picks shape 1, count0 = count1 - 1 the count just below the
    switch, n the smallest image count whose DENSE_PCT percent lie LIST_MARGIN pixels above count1.  None if there is none up to cap."""
    count1 = smallest_count_for_shape(1, cout, groups, n_simd, cap * hw * hw)
    if count1 is None or count1 < 2:
        return None
    for n in range(1, cap + 1):
        if list_is_followed(count1 + LIST_MARGIN, n * hw * hw):
            return n, count1, count1 - 1
    return None


def pixel_list(active_ids, mall):
    """The permutation svx_conv2d_same takes: the active pixel ids ascending, then all others ascending (int32 [mall])."""
    active = np.zeros(mall, bool)
    active[np.asarray(active_ids, np.int64)] = True
    return np.concatenate([np.flatnonzero(active), np.flatnonzero(~active)]).astype(np.int32)


# ---- svx_fc.hip ----
FC_RING = 6                         # weight ring: the loop body takes six octets, the tail Q % 6
FC_MIN_OCTETS = 24                  # octets a split holds at least


def fc_na(m, n):
    return 2 if (m > 64 and n % 64 == 0) else 1


def fc_instantiation(m, n):
    """(NA, NB) of the fc_splitk_kernel the entry point launches."""
    if fc_na(m, n) == 2:
        return (2, 2)
    return (1, 1) if m <= 32 else (1, 2)


def fc_row_tiles(m):
    return (m + 63) // 64


def fc_splits(m, n, k):
    tiles = (n // (32 * fc_na(m, n))) * fc_row_tiles(m)
    s = min((1024 + tiles - 1) // tiles, (k // 8) // FC_MIN_OCTETS)
    return max(s, 1)


def fc_q_lengths(m, n, k):
    """q1 - q0 of every split: the number of octets its k loop walks."""
    kq, s = k // 8, fc_splits(m, n, k)
    return [kq * (i + 1) // s - kq * i // s for i in range(s)]


# ---- the catalogue ----
# the two layers at which shape 1 is reached at each kernel size: (cin, cout, hw, ksize, groups)
SHAPE1_LAYERS = {
    "conv2 5x5 two groups": (96, 256, 27, 5, 2),
    "conv3 3x3 one group": (256, 384, 13, 3, 1),
}

# k-loop tail of the convolution, ksize 5: (name, n, cin, cout, h, w, groups)
CONV_TAIL_CASES = [
    ("cin_g 16: Q = 50, two octets in the tail", 2, 16, 64, 6, 7, 1),
    ("cin_g 32: Q = 100, one octet in the tail", 2, 32, 128, 5, 9, 1),
    ("cin_g 64 in two groups: Q = 200, two octets in the tail", 1, 128, 128, 7, 4, 2),
]

# grid sweep, 3x3, cin_g = 16: every (channels) x every (image)
GRID_CHANNELS = [                    # (name, cout, groups)
    ("one channel tile", 64, 1),
    ("three channel tiles: odd, eight pixel ranges", 192, 1),
    ("five channel tiles: odd, eight pixel ranges", 320, 1),
    ("two channel tiles: one per half", 128, 1),
    ("two groups of two tiles: a group per half", 256, 2),
    ("two groups of three tiles", 384, 2),
]
GRID_IMAGES = [                      # (name, n, h, w)
    ("M = 1: a single pixel", 1, 1, 1),
    ("M = 31: one short tile, one row", 1, 1, 31),
    ("M = 32: exactly one tile", 1, 4, 8),
    ("M = 33: one pixel into the second tile", 1, 3, 11),
    ("M = 95: five one-row images", 5, 1, 19),
    ("M = 96: three tiles", 1, 8, 12),
    ("M = 97: one column", 1, 97, 1),
    ("M = 255: three 5 x 17 images", 3, 5, 17),
    ("M = 256: eight tiles, one per pixel range", 1, 16, 16),
    ("M = 257: one column, nine tiles", 1, 257, 1),
    ("M = 1001: seven 11 x 13 images", 7, 11, 13),
]
GRID_CIN = 16

# one-hot probes on a 5 x 9 image: (batch, channel, y, x, ky, kx, out channel); cin 32, cout 128, two groups, n = 2
ONE_HOT_SHAPE = (2, 32, 128, 5, 9, 2)
ONE_HOT_PROBES = [
    ("tap (0, 2): lands one row down, one column left", 1, 5, 2, 7, 0, 2, 7),
    ("tap (2, 0): lands one row up, one column right", 0, 29, 4, 0, 2, 0, 100),
    ("tap (0, 2) at x = 8 > h: only a swap of H and W loses it", 1, 17, 0, 8, 0, 2, 70),
    ("tap (2, 0) from the last row: lands in the last column", 0, 3, 4, 7, 2, 0, 33),
]

# list mode at the tile edges: conv3-shaped, cin 32, n = 2, 13 x 13 (338 pixels)
LIST_EDGE_LAYER = (2, 32, 384, 13, 13, 3, 1)          # n, cin, cout, h, w, ksize, groups
LIST_EDGE_COUNTS = [0, 1, 31, 32, 33, 95, 96, 97]     # empty, one pixel, the edges of the 32- and the 96-pixel tile
LIST_FILL_REMAINDERS = [127, 128, 129]                # inactive pixels: one short copy unit, exactly one, one pixel into the second

# the 97 % rule: one 10 x 10 image, so that a count is a percentage
DENSE_RULE_LAYER = (1, 32, 64, 10, 10, 3, 1)
DENSE_RULE_COUNTS = [("96 %: the list is followed", 96, True), ("97 %: every pixel", 97, False), ("100 %", 100, False)]

# live in list mode
LIST_LIVE_LAYER = (6, 32, 64, 13, 13, 3, 1)
LIST_LIVE_VALUES = [1, 5, 6, 9]                       # (9 is clamped to n)

# fully connected: (name, m, n, k)
FC_TAIL_K = [8 * q for q in range(24, 30)]            # one split (k / 8 < 48), Q = 24 .. 29: every residue of 6
FC_TAIL_MN = [("<1,1>", 1, 32), ("<1,2>", 40, 32), ("<2,2>", 70, 64)]
FC_ROW_TILE_CASES = [
    ("<1,2>, two row tiles, three neuron tiles, ragged k", 65, 96, 1000),
    ("<1,2>, three row tiles, one neuron tile", 130, 32, 2048),
    ("row edge 32: the last row of <1,1>", 32, 64, 512),
    ("row edge 33: the first row of <1,2>'s second column", 33, 64, 512),
    ("row edge 64: a full <1,2> tile", 64, 64, 512),
    ("row edge 65: <2,2>, one row into the second tile", 65, 64, 512),
]
FC_LIVE_M, FC_LIVE_K = 130, 512
FC_LIVE_N = [64, 96]                                  # <2,2> and <1,2>
FC_LIVE_VALUES = [1, 32, 33, 64, 65, FC_LIVE_M, FC_LIVE_M + 7]


def fc_cases():
    """Every (m, n, k) the fc tests run."""
    out = [(m, n, k) for _name, m, n in FC_TAIL_MN for k in FC_TAIL_K]
    out += [(m, n, k) for _name, m, n, k in FC_ROW_TILE_CASES]
    out += [(FC_LIVE_M, n, FC_LIVE_K) for n in FC_LIVE_N]
    return out


# pooling + LRN: (name, radius, alpha, beta, k); radius None = the channel count (the window clamps at both ends everywhere)
POOL_PARAMS = [
    ("radius 0: the channel alone", 0, 2e-5, 0.75, 1.0),
    ("radius 1, beta 0.5, k 2: the powf branch", 1, 1e-4, 0.5, 2.0),
    ("radius 5, beta 1: the powf branch", 5, 2e-5, 1.0, 1.0),
    ("radius = C: clamps at both channel ends", None, 2e-5, 0.75, 1.0),
]
POOL_SHAPES = [                      # (name, n, C, H, W)
    ("one pooled pixel", 2, 8, 3, 3),
    ("even height and width", 1, 16, 4, 6),
    ("width 33: the row-mask shift reaches 32", 1, 24, 7, 33),
    ("even height and width, 96 channels", 2, 96, 12, 10),
]
POOL_SCALES = [30.0, 3000.0]

FC8_ROWS = [1, 64, 65]
