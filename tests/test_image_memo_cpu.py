"""CPU test of the image memo's key (svx_image_dedup, svision_amd/csrc/svx_raster_common.hpp image_key).

The key is restated here in Python from the device's line set-up (record_line: fp64 scaling, clipLine, LineIterator set-up)
and packed exactly as the device packs it.  What the memo relies on: records with equal keys give identical images from the
oracle's CPU rasteriser (oracle/encode_ref.py plot_pair_mask) -- on 10 k fuzzed records with planted look-alikes (fields
the scaling erases changed, fully clipped lines, pads) and on the image_small / collect_small fixtures.
"""
import gzip
import json
import os

import numpy as np

from oracle import encode_ref
from svision_amd.network import create_batch
from tests import datagen
from tests.helpers import GOLDEN

IMG = encode_ref.IMG
PAD = encode_ref.PAD_RECORD


def setup_line(x1, y1, x2, y2):
    """LineIterator(leftToRight) set-up of the device (svx_raster_common.hpp setup_line) -> (x0, y0, dx, dy, sy, steep, count)."""
    if not (0 <= x1 < IMG and 0 <= x2 < IMG and 0 <= y1 < IMG and 0 <= y2 < IMG):
        ok, x1, y1, x2, y2 = encode_ref.cv_clip_line(IMG, IMG, x1, y1, x2, y2)
        if not ok:
            return (0, 0, 0, 0, 1, 0, 0)
    dx, dy = x2 - x1, y2 - y1
    if dx < 0:
        dx, dy, x1, y1 = -dx, -dy, x2, y2
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = 1 if dy > dx else 0
    if steep:
        dx, dy = dy, dx
    return (x1, y1, dx, dy, sy, steep, dx + 1)


def record_line(r, s):
    """(Line, rev) of segment s of a 12-int record (svx_raster_common.hpp record_line)."""
    read_len, ref_len = int(r[10]), int(r[11])
    ratio = float(max(read_len, ref_len) / 227.0)
    if ratio < 1:
        ratio = 1.0
    xs, ys = int(r[5 * s]), int(r[5 * s + 2])
    length = int(r[5 * s + 3]) - ys
    fwd = int(r[5 * s + 4]) != 0
    xe = xs + (length - 1) if fwd else xs - (length - 1)
    ye = ys + (length - 1)
    cs, rs = int(float(ys) / ratio), int(float(xs) / ratio)
    ce, re_ = int(float(ye) / ratio), int(float(xe) / ratio)
    line = setup_line(cs, rs, ce, re_) if fwd else setup_line(ce, re_, cs, rs)
    return line, 0 if fwd else 1


def image_key(r):
    """The 128-bit key as four uint32 words, packed as the device packs it (include/svx.h svx_image_dedup)."""
    (l0, rev0), (l1, rev1) = record_line(r, 0), record_line(r, 1)
    words = [l[0] | l[1] << 8 | l[2] << 16 | l[3] << 24 for l in (l0, l1)]
    flags = [(1 if l[4] < 0 else 0) | l[5] << 1 | rev << 2 for l, rev in ((l0, rev0), (l1, rev1))]
    return (words[0], words[1], flags[0] | flags[1] << 8, l0[6] | l1[6] << 16)


def keys_of(records):
    return np.asarray([image_key(r) for r in records], np.uint64).astype(np.uint32)


def planted(seed=5, n=10_000):
    """Fuzzed records with look-alikes planted next to their originals: fields the scaling erases changed (read / ref length,
    the stored x end, coordinates moved below the scale), fully clipped lines, pads."""
    rng = np.random.default_rng(seed)
    base = datagen.random_records(n // 2, seed=seed, hostile=True).astype(np.int64)
    out = [base]
    alt = base.copy()
    for i in range(alt.shape[0]):
        r = alt[i]
        kind = i % 5
        ratio = max(r[10], r[11]) / 227.0
        if kind == 0:                                         # the stored x end is never read
            r[1] += int(rng.integers(-1000, 1000)); r[6] += int(rng.integers(-1000, 1000))
        elif kind == 1 and ratio > 4:                         # a coordinate moved by less than a pixel of the scale (may or may not cross)
            r[0] += int(rng.integers(0, 2)); r[7] += int(rng.integers(0, 2))
        elif kind == 2:                                       # the shorter of the two lengths changes nothing while it stays shorter
            j = 10 if r[10] < r[11] else 11
            r[j] = int(rng.integers(1, max(r[10], r[11]) + 1))
        elif kind == 3:                                       # both segments far outside the image: fully clipped
            for k in (0, 5):
                r[k] = -10 * (max(r[10], r[11]) + 300); r[k + 1] = r[k]
                r[k + 2] = int(rng.integers(0, 10)); r[k + 3] = r[k + 2] + int(rng.integers(1, 50))
        else:
            r[:] = PAD
    out.append(alt)
    recs = np.concatenate(out)
    recs = recs[rng.permutation(recs.shape[0])]
    return np.clip(recs, np.iinfo(np.int32).min, np.iinfo(np.int32).max).astype(np.int32)


def fixture_records():
    with gzip.open(os.path.join(GOLDEN, "image_small.expected.json.gz"), "rb") as f:
        doc = json.load(f)
    img = np.asarray([create_batch.parse_data_fields(d.split("_")) for d in doc["data"]], np.int32)
    with open(os.path.join(GOLDEN, "collect_small.expected.json")) as f:
        coll = json.load(f)
    lines = [ln for w in coll["windows"] for ln in w["tsv"].splitlines() if ln]
    col = np.asarray([encode_ref.parse_tsv_line(ln)[0] for ln in lines], np.int32)
    return img, col


def check_equal_keys_equal_images(records):
    """Every group of records with one key rasterises to one image; returns (records, distinct keys)."""
    keys = keys_of(records)
    _u, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    cache = {}
    for i in range(records.shape[0]):
        g = int(inverse[i])
        if int(first[g]) == i:
            continue                                          # a group's own first member: compared by the others
        if g not in cache:
            cache[g] = encode_ref.plot_pair_mask(records[first[g]])
        assert np.array_equal(encode_ref.plot_pair_mask(records[i]), cache[g]), (records[i], records[first[g]])
    return records.shape[0], len(first)


def test_key_packs_the_line_setup_losslessly():
    recs = datagen.random_records(2000, seed=9, hostile=True)
    for r in recs:
        (l0, rev0), (l1, rev1) = record_line(r, 0), record_line(r, 1)
        for l in (l0, l1):
            x0, y0, dx, dy, sy, steep, count = l
            assert all(0 <= v < IMG for v in (x0, y0, dx, dy)) and 0 <= count <= IMG and sy in (-1, 1)
            assert count == (dx + 1 if count else 0)
        k = image_key(r)
        unpack = [((k[s] >> (8 * j)) & 255) for s in (0, 1) for j in range(4)]
        assert unpack == [l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]]
        assert (k[2] & 255, k[2] >> 8, k[3] & 0xFFFF, k[3] >> 16) == (
            (l0[4] < 0) | l0[5] << 1 | rev0 << 2, (l1[4] < 0) | l1[5] << 1 | rev1 << 2, l0[6], l1[6])


def test_equal_keys_give_identical_images_on_planted_fuzz():
    recs = planted()
    n, distinct = check_equal_keys_equal_images(recs)
    assert n == 10_000 and distinct < 0.8 * n                 # the look-alikes did collapse


def test_equal_keys_give_identical_images_on_the_fixtures():
    img, col = fixture_records()
    for recs in (img, col):
        n, distinct = check_equal_keys_equal_images(recs)
        assert 0 < distinct < n
    pads = np.asarray([PAD] * 3, np.int32)
    assert len(set(map(tuple, keys_of(pads)))) == 1

