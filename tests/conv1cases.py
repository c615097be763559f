"""Crafted similarity images for the sparse first layer and the active-pixel lists, and what they must give.

Plain Python and NumPy: no torch, no product import.  The first part builds records whose images single out what a random image does not
(tests/test_gpu_conv1_cases.py runs them, tests/test_conv1cases_cpu.py proves with the Python oracle that each contains what it claims):

  a  one-pixel probes at every column of rows 0, 113, 226 and at every row of columns 0, 113, 226: every bit offset and word boundary
     of ``window_mask`` (svision_amd/csrc/svx_cnn.hip) in the bit planes and in ``rowany``, the first and the last conv window, the word
     behind ``colmask``;
  b  two pixels in one column, 1, 4, 11, 19 and 190 rows apart, at columns 0, 21, 22, 31, 32 and 226: channel 1 (= channel 0 restricted to
     the columns with two hits) inside one window, in the neighbouring window and in a strip another workgroup owns;
  c  the two diagonals, each diagonal alone, a 19-pixel cross on pixel (113, 113) and two pixels in row 113: pooled pixels with nine,
     eight and fewer non-empty conv windows under them;
  d  the empty image first, in the middle and last, and the padding record.

A record cannot draw a vertical or a horizontal line: both coordinates of a segment advance by the same length (create_batch.py:118,132 of
the reference, oracle/encode_ref.record_segments), and one ratio scales both.  Group b holds the vertical pairs, group c a horizontal one.

The second part RESTATES, in float64 / on boolean arrays, what the two entry points claim: conv1 of the 0 / 255 image without the mean
cancellation (base[k] + 255 * the weight rows of the set pixels), ReLU, the 3x3/2 max-pool and TensorFlow's LRN; the rounding bound of the
kernel's sequential fmaf chain; the touched pixels; and the dilation / pooling chain that turns them into the pixel lists of conv2..conv5.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import encode_ref

IMG, C1, CONV1, P1, A2 = 227, 96, 55, 27, 13
DENSE_PCT = 97                       # include/svx.h SVX_CONV_DENSE_PCT
SEQ_TERMS = 364                      # base + 11 * 11 * 3 taps: the longest fmaf chain of one lane
UNIT = 2.0 ** -24                    # unit roundoff of float32

# ---- records ----
OFF = (100000, 100001, 100000, 100001, 1)            # a segment far outside the image: clipLine drops it


def pixel(r, c, fwd=1):
    """The segment that draws the single pixel (row r, col c); a reverse one also sets channel 2."""
    return (r, r + 1, c, c + 1, fwd)


def record(seg_a, seg_b, length=IMG):
    """Two segments and read_len = ref_len = length (227 or 1: ratio 1 either way)."""
    return tuple(seg_a) + tuple(seg_b) + (length, length)


Case = namedtuple("Case", "group name rec counts")    # counts: set pixels in channels 0, 1, 2

EMPTY = Case("d", "empty image", record(OFF, OFF), (0, 0, 0))
PAD = Case("d", "padding record", tuple(encode_ref.PAD_RECORD), (2, 0, 0))
PROBE_LINES = (0, 113, 226)
PAIR_GAPS = (1, 4, 11, 19, 190)
PAIR_COLS = (0, 21, 22, 31, 32, 226)
DIAG_FWD, DIAG_REV = (0, 227, 0, 227, 1), (226, 453, 0, 227, 0)


def _group_a():
    out = []
    spots = [(r, c) for r in PROBE_LINES for c in range(IMG)] + [(r, c) for c in PROBE_LINES for r in range(IMG)]
    for i, (r, c) in enumerate(spots):
        fwd = 1 - (i & 1)                              # forward and reverse alternate
        twice = (i >> 1) & 1                           # the pixel given twice, or paired with a segment off the image
        length = 1 if (i >> 2) & 1 else IMG
        rec = record(pixel(r, c, fwd), pixel(r, c, fwd) if twice else OFF, length)
        out.append(Case("a", "pixel (%d, %d) %s" % (r, c, "fwd" if fwd else "rev"), rec, (1, 0, 0 if fwd else 1)))
    return out


def _group_b():
    out = []
    for ci, c in enumerate(PAIR_COLS):
        for gi, gap in enumerate(PAIR_GAPS):
            r1 = 10 + ci                               # (10, 200) at column 31 is the pair (13, 203) here; rows differ per column
            fwd2 = (ci + gi) & 1                       # a reverse second segment sets channel 2 at its own pixel only
            out.append(Case("b", "column %d rows %d and %d" % (c, r1, r1 + gap), record(pixel(r1, c, 1), pixel(r1 + gap, c, fwd2)),
                            (2, 2, 0 if fwd2 else 1)))
    return out


def _group_c():
    return [
        Case("c", "two diagonals", record(DIAG_FWD, DIAG_REV), (453, 452, 227)),
        Case("c", "forward diagonal", record(DIAG_FWD, OFF), (227, 0, 0)),
        Case("c", "reverse diagonal", record(OFF, DIAG_REV), (227, 0, 227)),
        Case("c", "cross on (113, 113)", record((104, 123, 104, 123, 1), (122, 141, 104, 123, 0)), (37, 36, 19)),
        Case("c", "two pixels in row 113", record(pixel(113, 113, 1), pixel(113, 150, 0)), (2, 0, 1)),
    ]


@functools.lru_cache(maxsize=None)
def cases():
    """The whole table in launch order: the empty image first, in the middle and last."""
    return tuple([EMPTY] + _group_a() + _group_b() + [EMPTY] + _group_c() + [PAD, EMPTY])


def records(table=None):
    return np.asarray([c.rec for c in (cases() if table is None else table)], np.int32).reshape(-1, 12)


def group_ids(group):
    return [i for i, c in enumerate(cases()) if c.group == group]


def empty_ids():
    return [i for i, c in enumerate(cases()) if c is EMPTY]


def mixed_ids():
    """About 40 cases of every kind, for the launches that are repeated (LRN parameters, live counts): the empty image first,
    inside and last, the padding record, groups b and c, and the probes at the corners, the centre and the word boundaries."""
    t = cases()
    a = {c.name.rsplit(" ", 1)[0]: i for i, c in enumerate(t) if c.group == "a"}
    probes = [a["pixel (%d, %d)" % rc] for rc in ((0, 0), (0, 21), (0, 22), (0, 31), (0, 32), (0, 226), (113, 113), (226, 0), (226, 226),
                                                  (113, 63), (113, 64), (31, 113), (32, 113), (225, 226))]
    e = empty_ids()
    ids = [e[0]] + probes + group_ids("b")[::2] + [e[1]] + group_ids("c") + [i for i, c in enumerate(t) if c is PAD] + [e[2]]
    assert len(set(ids)) == len(ids)
    return ids


# ---- the image, from the Python oracle ----
@functools.lru_cache(maxsize=None)
def _table_masks():
    return oracle_masks(records())


def oracle_masks(rec):
    """bool [n, 227, 227, 3]: the pixels oracle/encode_ref draws.  ``rec`` None: the whole table (cached, read only)."""
    if rec is None:
        return _table_masks()
    out = np.stack([encode_ref.plot_pair_mask(r) for r in np.asarray(rec).reshape(-1, 12)]) != 0
    out.setflags(write=False)
    return out


def window_nonempty(mask):
    """bool [n, 55, 55]: conv1 window (oy, ox) -- image rows 4oy .. 4oy+10, columns 4ox .. 4ox+10 -- holds a set pixel in some channel."""
    on = mask.any(3)
    cols = np.stack([on[:, :, 4 * x:4 * x + 11].any(2) for x in range(CONV1)], 2)
    return np.stack([cols[:, 4 * y:4 * y + 11, :].any(1) for y in range(CONV1)], 1)


def window_census(mask):
    """int [n, 27, 27]: how many of the nine conv windows under a pooled pixel are non-empty."""
    ne = window_nonempty(mask).astype(np.int64)
    return sum(ne[:, dy:dy + 2 * P1 - 1:2, dx:dx + 2 * P1 - 1:2] for dy in range(3) for dx in range(3))


def touched_pixels(mask):
    """bool [n, 27, 27]: pooled pixels with a set pixel in their receptive field, image rows 8py .. 8py+18, columns 8px .. 8px+18
    (touched_from_pixels of tests/test_image_golden.py on whole arrays)."""
    on = mask.any(3)
    cols = np.stack([on[:, :, 8 * x:8 * x + 19].any(2) for x in range(P1)], 2)
    return np.stack([cols[:, 8 * y:8 * y + 19, :].any(1) for y in range(P1)], 1)


def to_words(b):
    """bool [..., rows, width] -> uint32 [..., rows]: bit x of word y = pixel (y, x).  Bits 27 .. 31 of a touched word are outside
    what include/svx.h defines; they stay clear here."""
    return (b.astype(np.uint64) << np.arange(b.shape[-1], dtype=np.uint64)).sum(-1).astype(np.uint32)


def from_words(w, width=P1):
    return ((np.asarray(w).astype(np.int64)[..., None] >> np.arange(width)) & 1).astype(bool)


# ---- weights ----
def weights_a(seed=3):
    """randn * 0.01 weights and a randn base: the scale of tests/test_image_golden.py."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((11, 11, 3, C1)) * 0.01).astype(np.float32), rng.standard_normal(C1).astype(np.float32)


def weights_b(seed=4):
    """Channels 0 .. 47: base +50 and all weights negative -- every set tap lowers a window's response, so a pooled pixel whose nine
    windows are all non-empty comes out BELOW relu(base), and one with an empty window at exactly relu(base).  Channels 48 .. 95: base
    -50 and all weights positive -- an empty window gives 0, a window with enough taps a positive value."""
    rng = np.random.default_rng(seed)
    mag = (0.002 + np.abs(rng.standard_normal((11, 11, 3, C1))) * 0.01).astype(np.float32)
    sign = np.where(np.arange(C1) < C1 // 2, -1.0, 1.0).astype(np.float32)
    return mag * sign, (-50.0 * sign).astype(np.float32)


WEIGHTS = {"A": weights_a, "B": weights_b}


# ---- fp64 restatements of the layer ----
def max_pool(x):
    """3x3 stride-2 VALID max-pool of [n, H, W, C]."""
    oh, ow = (x.shape[1] - 3) // 2 + 1, (x.shape[2] - 3) // 2 + 1
    out = None
    for dy in range(3):
        for dx in range(3):
            v = x[:, dy:dy + 2 * oh - 1:2, dx:dx + 2 * ow - 1:2]
            out = v if out is None else np.maximum(out, v)
    return out


def conv1_ref64(mask, w1, base):
    """(pooled, bound), float64 [n, 27, 27, 96] each, from the float32 w1 (HWIO) and base.
    pooled = max-pool(relu(base[k] + 255 * sum of w1 over the set taps of the window)).
    bound: a lane adds at most 363 terms to base by sequential fmaf, so a window's response is within SEQ_TERMS * 2^-24 * S of the
    exact one, S = |base[k]| + 255 * sum |w1| over the window's set taps; ReLU is 1-Lipschitz and |max a_i - max b_i| <= max |a_i - b_i|,
    so the pooled value is within the max-pool of that."""
    n = mask.shape[0]
    m = np.ascontiguousarray(mask, np.float64)
    s0, s1, s2, s3 = m.strides
    cols = np.lib.stride_tricks.as_strided(m, (n, CONV1, CONV1, 11, 11, 3), (s0, 4 * s1, 4 * s2, s1, s2, s3), writeable=False)
    cols = cols.reshape(n * CONV1 * CONV1, 363)
    w = w1.astype(np.float64).reshape(363, C1)
    b = base.astype(np.float64)
    conv = (b + 255.0 * (cols @ w)).reshape(n, CONV1, CONV1, C1)
    s = (np.abs(b) + 255.0 * (cols @ np.abs(w))).reshape(n, CONV1, CONV1, C1)
    return max_pool(np.maximum(conv, 0.0)), SEQ_TERMS * UNIT * max_pool(s)


def lrn64(x, radius=2, alpha=2e-05, beta=0.75, k=1.0):
    """oracle/alexnet_ref._lrn kept in float64: x / (k + alpha * sum_{|j - c| <= radius} x_j^2)^beta over the last axis."""
    x = np.asarray(x, np.float64)
    sq = np.square(x)
    c = x.shape[-1]
    acc = np.zeros_like(x)
    for d in range(-min(radius, c), min(radius, c) + 1):
        lo, hi = max(0, d), min(c, c + d)
        acc[..., lo - d:hi - d] += sq[..., lo:hi]
    return x / np.power(k + alpha * acc, beta)


LRN_DEFAULT = ("the network's: radius 2, alpha 2e-5, beta 0.75, k 1", 2, 2e-5, 0.75, 1.0)


def lrn_params():
    """Every row of cnncases.POOL_PARAMS (radius None -> 96) and the defaults."""
    from tests import cnncases
    return [LRN_DEFAULT] + [(name, C1 if radius is None else radius, alpha, beta, k) for name, radius, alpha, beta, k in cnncases.POOL_PARAMS]


# ---- the active sets ----
def dilate(m, r):
    """Boolean [..., H, W] dilated by a (2r + 1) x (2r + 1) window."""
    out = np.zeros_like(m)
    h, w = m.shape[-2:]
    pad = np.pad(m, [(0, 0)] * (m.ndim - 2) + [(r, r), (r, r)])
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[..., dy:dy + h, dx:dx + w]
    return out


def pool_any(a):
    """Boolean [n, 27, 27] -> [n, 13, 13]: a 3x3 stride-2 VALID window holds an active pixel."""
    n, h, w = a.shape
    oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    out = np.zeros((n, oh, ow), bool)
    for y in range(oh):
        for x in range(ow):
            out[:, y, x] = a[:, 2 * y:2 * y + 3, 2 * x:2 * x + 3].any((1, 2))
    return out


def active_masks(touched):
    """touched bool [n, 27, 27] -> the active output pixels of conv2 [n, 27, 27] and conv3, conv4, conv5 [n, 13, 13]."""
    a2 = dilate(touched, 2)
    a3 = dilate(pool_any(a2), 1)
    a4 = dilate(a3, 1)
    a5 = dilate(a4, 1)
    return a2, a3, a4, a5


def pixel_list(mask):
    """The permutation of one layer: the active pixel ids ascending, then the others ascending (image * H*W + y * W + x)."""
    flat = mask.reshape(-1)
    return np.concatenate([np.flatnonzero(flat), np.flatnonzero(~flat)]).astype(np.int32)


def executed(total, every):
    """What svx_conv2d_same computes given a list with ``total`` of ``every`` pixels active: all of them from DENSE_PCT percent on."""
    return every if total * 100 >= every * DENSE_PCT else total


def expected_active_sets(touched, live=None):
    """What one launch over touched bool [n, 27, 27] must give: the four lists over the leading min(live, n) images, their counts,
    conv2's row masks of those images, and what the launch adds to the five running totals."""
    n = touched.shape[0]
    m = n if live is None else min(live, n)
    masks = active_masks(touched[:m])
    lists = [pixel_list(a) for a in masks]
    counts = [int(a.sum()) for a in masks]
    add = [executed(c, a.size) for c, a in zip(counts, masks)] + [n]
    return lists, counts, to_words(masks[0]), add


def single_bit_touched():
    """729 images with one touched pixel each, image y * 27 + x at (y, x): more images than the lists kernel has threads."""
    t = np.zeros((P1 * P1, P1, P1), bool)
    i = np.arange(P1 * P1)
    t[i, i // P1, i % P1] = True
    return t


SINGLE_CUTS = (1, 255, 256, 257, 729)                 # around the 256 threads of the prefix loop, and the whole set


def empty_and_full_touched():
    """Empty, full, empty, full, full: counts 0 and H*W, an inactive image in front of an active one."""
    t = np.zeros((5, P1, P1), bool)
    t[[1, 3, 4]] = True
    return t


def threshold_touched(below, n=4):
    """n - 1 full images and one partial image in the middle whose conv2 set misses as many pixels as DENSE_PCT allows (below = 0: the
    list is exactly DENSE_PCT percent full and svx_conv2d_same computes every pixel) or one more (below = 1: the list is followed).
    The inactive conv2 pixels are a prefix of the image in row-major order; the untouched first-layer pixels are that prefix dilated."""
    every = n * P1 * P1
    miss = every - -(-every * DENSE_PCT // 100) + below        # every - ceil(every * DENSE_PCT / 100)
    inactive = (np.arange(P1 * P1) < miss).reshape(P1, P1)
    t = np.ones((n, P1, P1), bool)
    t[n // 2] = ~dilate(inactive, 2)
    return t, every - miss


def live_values(n):
    return sorted({0, 1, n - 1, n, n + 5} - {-1})
