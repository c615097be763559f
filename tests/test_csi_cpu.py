"""svision_amd/io/csi.py against tests/csilike.py (a second reading of the CSI layout that shares no code with it): the bins, the
depth, the writer byte for byte, the container, the reader on its own files and on what other writers leave, the two bounds the
device decoder cuts its slices with, and the refusal of a ``.bai`` for positions from 2^29 on.  No GPU, no file of the project's
native library: record lists with made-up virtual offsets."""
import gzip
import os

import numpy as np
import pytest

from svision_amd.io import bai, bam, csi
from tests import baicases, csilike, htslike

EDGE = 1 << 29


def _arrays(references, records, voffs):
    pos = np.asarray([r["pos"] for r in records], np.int64)
    end = pos + np.asarray([htslike.ref_len(r.get("cigar", [])) or 1 for r in records], np.int64)
    return (len(references), [l for _n, l in references], np.asarray([r["tid"] for r in records], np.int64), pos, end,
            np.asarray([r["flag"] for r in records], np.int64), np.asarray(voffs[:-1], np.uint64), np.asarray(voffs[1:], np.uint64))


def _lists():
    return {"short": (baicases.REFS, baicases.short_records(n=120)), "cg": (baicases.REFS, baicases.short_records(seed=4, n=60, cg=True)),
            "ont": (baicases.REFS, baicases.long_records()), "long": (csilike.LONG_REFS, csilike.long_records())}


@pytest.fixture(scope="module")
def cases():
    """name -> (references, records, voffs, the arguments of csi_bytes)"""
    out = {}
    for k, (refs, recs) in _lists().items():
        recs = [dict(r, seq="*", qual=None) for r in recs]      # (the index does not read bases)
        voffs = csilike.fake_voffs(recs, seed=len(k))
        out[k] = (refs, recs, voffs, _arrays(refs, recs, voffs))
    return out


_as_idx = csilike.as_idx


# ---- bins and depth -----------------------------------------------------------------------------------------------------------
def test_reg2bin_exhaustive_small():
    """(min_shift, depth) = (2, 2), every interval of a 256-base reference: the loop's bin, and that bin is the smallest that holds it."""
    beg, end = np.asarray([(b, e) for b in range(256) for e in range(b + 1, 257)]).T
    got = csi.reg2bin(beg, end, 2, 2)
    assert got.tolist() == [csilike.reg2bin(int(b), int(e), 2, 2) for b, e in zip(beg, end)]
    level = csi.bin_level(got)
    size = 1 << (2 + 3 * (2 - level))
    start = csi.bin_first_window(got, 2) << 2
    assert ((start <= beg) & (end <= start + size)).all()
    deeper = level < 2                                          # no bin one level down holds it
    assert ((beg[deeper] // (size[deeper] >> 3)) != ((end[deeper] - 1) // (size[deeper] >> 3))).all()
    assert csi.bin_level([0, 1, 8, 9, 72, 73, 584, 585]).tolist() == [0, 1, 1, 2, 2, 3, 3, 4]


def test_reg2bin_random():
    rng = np.random.default_rng(11)
    beg = rng.integers(0, EDGE - 1, 4000)
    end = np.minimum(beg + rng.choice([1, 2, 300, 16384, 20_000, 1 << 20, 1 << 27], 4000), EDGE)
    assert (csi.reg2bin(beg, end, 14, 5) == bai.reg2bin(beg, end)).all()
    assert (csi.reg2bin(beg, end) == bai.reg2bin(beg, end)).all()
    for min_shift, depth in ((14, 6), (12, 3)):
        top = 1 << (min_shift + 3 * depth)
        beg = rng.integers(0, top - 1, 3000)
        beg[:6] = [0, top - 1, EDGE - 1, EDGE, EDGE - 5, 1][:6]
        beg = np.minimum(beg, top - 1)
        end = np.minimum(beg + rng.choice([1, 2, 300, 4096, 4097, 16384, 20_000, 1 << 20, 1 << 27], 3000), top)
        assert csi.reg2bin(beg, end, min_shift, depth).tolist() == [csilike.reg2bin(int(b), int(e), min_shift, depth) for b, e in zip(beg, end)]


def test_depth_for():
    assert [csi.depth_for(v) for v in (EDGE - 257, EDGE - 256, EDGE - 255, 1 << 32, 600_000)] == [5, 5, 6, 7, 2]
    assert csi.depth_for(600_000, 12) == 3 and csi.depth_for(0) == 0 and csi.depth_for(700_000_000) == 6
    assert csi.meta_bin(5) == bai.META_BIN


# ---- the writer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["short", "cg", "ont", "long"])
def test_payload_equals_csilike(cases, name):
    refs, recs, voffs, args = cases[name]
    data = csi.csi_bytes(*args)
    want = csilike.payload(refs, recs, voffs)
    assert csilike.inflate(data) == want == csi.csi_payload(*args)
    idx = csilike.parse(want)
    assert idx["depth"] == (6 if name == "long" else 2) and idx["min_shift"] == 14 and idx["n_no_coor"] == sum(r["tid"] < 0 for r in recs)
    # the container: members a gzip reader takes, none above 0xFF00 inflated bytes, the end-of-file marker last
    assert gzip.decompress(data) == want and data.endswith(csilike.EOF_BLOCK)
    members, at = 0, 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00"
        bsize = int.from_bytes(data[at + 16:at + 18], "little") + 1
        assert int.from_bytes(data[at + bsize - 4:at + bsize], "little") <= 0xFF00
        at, members = at + bsize, members + 1
    assert at == len(data) and members == -(-len(want) // 0xFF00) + 1


def test_other_min_shift_and_depth(cases):
    refs, recs, voffs, args = cases["short"]
    for min_shift, depth in ((12, None), (14, 4), (10, 5)):
        assert csi.csi_payload(*args, min_shift=min_shift, depth=depth) == csilike.payload(refs, recs, voffs, min_shift, depth)
    assert csilike.parse(csi.csi_payload(*args, min_shift=12))["depth"] == 3


def test_writer_refuses(cases):
    refs, recs, voffs, args = cases["long"]
    with pytest.raises(ValueError, match="cannot hold positions from %d on" % EDGE):
        csi.csi_bytes(*args, depth=5)
    n_ref, lengths, tid, pos, end, flag, voff, voff_end = args
    with pytest.raises(ValueError, match="names reference 2 of 2"):
        csi.csi_bytes(n_ref, lengths, np.where(tid == 1, 2, tid), pos, end, flag, voff, voff_end)
    swapped = pos.copy()
    swapped[[3, 4]] = swapped[[4, 3]] if pos[3] != pos[4] else [pos[4] + 1, pos[3]]
    with pytest.raises(ValueError, match="not coordinate-sorted"):
        csi.csi_bytes(n_ref, lengths, tid, swapped, end, flag, voff, voff_end)


# ---- the reader ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["short", "ont", "long"])
def test_read_csi_round_trip_and_regions(cases, name, tmp_path):
    refs, recs, voffs, args = cases[name]
    path = str(tmp_path / "own.csi")
    with open(path, "wb") as f:
        f.write(csi.csi_bytes(*args))
    got = csi.read_csi(path)
    assert _as_idx(got) == csilike.parse(csilike.payload(refs, recs, voffs)) and got.aux == b""
    idx = _as_idx(got)
    for t, beg, end in csilike.regions(refs, recs, 500, seed=5):
        assert csilike.reached(idx, recs, voffs, t, beg, end) == csilike.brute(recs, t, beg, end), (t, beg, end)


@pytest.mark.parametrize("name", ["short", "long"])
@pytest.mark.parametrize("member", [None, 0xFF00, 700])
def test_reader_on_a_foreign_file(cases, name, member, tmp_path):
    """What other writers leave: loffsets that are lower bounds only or 0, merged chunks, a reference without the pseudo-bin, no
    n_no_coor, 28 aux bytes; one gzip member, BGZF members, many small ones."""
    refs, recs, voffs, _args = cases[name]
    want = csilike.payload(refs, recs, voffs, foreign=True)
    path = str(tmp_path / "foreign.csi")
    with open(path, "wb") as f:
        f.write(csilike.container(want, member, eof=member != 700))
    got = csi.read_csi(path)
    assert _as_idx(got) == csilike.parse(want)
    assert got.aux == csilike.AUX and got.n_no_coor is None and got.meta[0] is not None and got.meta[len(refs) - 1] is None
    assert any(l == 0 for bins in got.bins for _b, l, _c in bins)
    idx = _as_idx(got)
    for t, beg, end in csilike.regions(refs, recs, 500, seed=6):
        assert csilike.reached(idx, recs, voffs, t, beg, end) == csilike.brute(recs, t, beg, end), (t, beg, end)
    assert csi.index_format(path) == "csi"
    own = csi.spans(path)
    first = [min(v for v, r in zip(voffs, recs) if r["tid"] == t) for t in (0, len(refs) - 1)]
    assert [own[0][0], own[len(refs) - 1][0]] == first


def test_read_csi_refuses(cases, tmp_path):
    refs, recs, voffs, args = cases["short"]
    want = csi.csi_payload(*args)
    path = str(tmp_path / "bad.csi")

    def refused(data, match, raw=False):
        with open(path, "wb") as f:
            f.write(data if raw else csilike.container(data))
        with pytest.raises(ValueError, match=match) as exc:
            csi.read_csi(path)
        assert path in str(exc.value)
    refused(b"CSJ\x01" + want[4:], "not a CSI index")
    refused(want[:len(want) // 2], "is cut")
    refused(csi.csi_bytes(*args)[:200], "does not inflate", raw=True)
    refused(b"BAI\x01" + want[4:], "does not inflate", raw=True)
    at = 16 + 4 + 4                                             # the first bin number of the first reference
    refused(want[:at] + (csi.meta_bin(2) + 5).to_bytes(4, "little") + want[at + 4:], "outside depth 2")


# ---- the device decoder's two bounds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("foreign", [False, True])
@pytest.mark.parametrize("name", ["short", "ont", "long"])
def test_from_voff_to_voff_invariants(cases, name, foreign, tmp_path):
    """At every 16 kb boundary P of every reference: every record that reaches beyond P lies at or behind from_voff(P), every record
    that starts in front of P lies in front of to_voff(P); the seeds are record starts, the first record's among them."""
    refs, recs, voffs, args = cases[name]
    path = str(tmp_path / "x.csi")
    with open(path, "wb") as f:
        f.write(csilike.container(csilike.payload(refs, recs, voffs, foreign=True)) if foreign else csi.csi_bytes(*args))
    spans = csi.spans(path, decoder=True)
    _n, _l, tid, pos, end, _f, voff, voff_end = args
    assert spans[1] is None if name != "long" else spans[1] is not None
    for t, span in enumerate(spans):
        if span is None:
            continue
        rows = np.flatnonzero(tid == t)
        v, p, e = voff[rows].astype(np.int64), pos[rows], end[rows]
        assert span.usable and (span.lo, span.hi) == (int(v[0]), int(voff_end[rows[-1]])) == (span[0], span[1])
        assert set(span.seeds.tolist()) <= set(v.tolist()) and int(v[0]) in span.seeds.tolist() and (np.diff(span.seeds.astype(np.int64)) > 0).all()
        tight = 0
        for P in range(0, refs[t][1] + 2 * 16384, 16384):
            left, right = span.from_voff(P), span.to_voff(P)
            beyond, before = v[e > P], v[p < P]
            assert span.lo <= left <= span.hi and span.lo <= right <= span.hi
            assert beyond.size == 0 or left <= beyond.min(), (t, P)
            assert before.size == 0 or right > before.max(), (t, P)
            tight += beyond.size > 0 and left == beyond.min()
        assert span.from_voff(-5) == span.lo and span.to_voff(refs[t][1] + (1 << 20)) == span.hi
        assert tight > 0 or foreign                            # (the project's own loffsets are the linear index: met exactly somewhere)
        # the look-up a slice without a record falls back on: the next record start the index names
        assert span.next_behind(0, span.lo) == (int(span.seeds[1]) if span.seeds.size > 1 else span.hi)


def test_spans_of_both_formats(cases, tmp_path):
    refs, recs, voffs, args = cases["short"]
    n_ref, _lengths, *rest = args
    paths = {}
    for k, data in (("bai", bai.bai_bytes(n_ref, *rest)), ("csi", csi.csi_bytes(*args)), ("csi12", csi.csi_bytes(*args, min_shift=12))):
        paths[k] = str(tmp_path / ("x." + k))
        with open(paths[k], "wb") as f:
            f.write(data)
    assert [csi.index_format(paths[k]) for k in ("bai", "csi", "csi12")] == ["bai", "csi", "csi"]
    want = bam.read_bai(paths["bai"])
    assert csi.spans(paths["bai"]) == want == csi.spans(paths["csi"]) == csi.spans(paths["csi12"]) and want[1] is None
    lin, dec, dec12 = csi.spans(paths["bai"], decoder=True), csi.spans(paths["csi"], decoder=True), csi.spans(paths["csi12"], decoder=True)
    assert isinstance(lin[0], csi.LinearSpan) and isinstance(dec[0], csi.CsiSpan) and lin[1] is dec[1] is None
    assert lin[0].usable and dec[0].usable and not dec12[0].usable and dec12[0].min_shift == 12
    assert (lin[0].lo, lin[0].hi) == (dec[0].lo, dec[0].hi) == want[0]
    # the .bai road is its linear index, unchanged; a .csi of the project's own is as tight on the left wherever a bin starts
    raw = bam.read_bai_linear(paths["bai"])[0]
    assert (lin[0].seeds == raw[2]).all() and all(lin[0].from_voff(P) == lin[0].to_voff(P) == csi.voff_at(raw, P) for P in range(-16384, 500_000, 5_000))
    assert all(dec[0].from_voff(P) <= lin[0].from_voff(P) for P in range(0, 400_000, 16384))
    with open(paths["bai"], "wb") as f:
        f.write(b"nothing of the kind")
    with pytest.raises(ValueError, match="neither a BAI nor a CSI"):
        csi.spans(paths["bai"])


def test_find_index_precedence(tmp_path):
    path = str(tmp_path / "s.bam")
    assert bam.find_index(path) is None
    order = [str(tmp_path / "s.csi"), path + ".csi", str(tmp_path / "s.bai"), path + ".bai"]
    for p in order:                                             # each one written wins over those before it
        open(p, "wb").close()
        assert bam.find_index(path) == p
    os.unlink(path + ".bai")
    os.unlink(str(tmp_path / "s.bai"))
    assert bam.find_index(path) == path + ".csi"


# ---- a .bai cannot hold positions from 2^29 on ------------------------------------------------------------------------------------
def test_bai_refuses_from_2_29_on():
    def build(pos, end):
        return bai.bai_bytes(1, [0, 0], [100, pos], [200, end], [0, 0], [1 << 16, 2 << 16], [2 << 16, 3 << 16])
    assert build(EDGE - 50, EDGE)[:4] == b"BAI\x01"              # its last base is 2^29 - 1
    for pos, end in ((EDGE - 50, EDGE + 1), (EDGE, EDGE + 1), (EDGE + 7, EDGE + 7)):
        with pytest.raises(ValueError, match=r"a \.bai cannot hold positions from 2\^29 on") as exc:
            build(pos, end)
        assert isinstance(exc.value, bai.TooLong) and (exc.value.tid, exc.value.pos) == (0, pos) and str(pos) in str(exc.value)
    # a record without a reference has no position to refuse
    assert bai.bai_bytes(1, [0, -1], [100, EDGE + 5], [200, EDGE + 6], [0, 4], [1 << 16, 2 << 16], [2 << 16, 3 << 16])[:4] == b"BAI\x01"


def test_callers_name_reference_position_and_switch():
    from svision_amd import index
    exc = bai.TooLong(0, EDGE + 3, EDGE + 9, "a .bai cannot hold positions from 2^29 on")
    text = index.too_long_message(exc, ["long", "chrB"], "write a .csi instead: --csi (SVX_BUILD_INDEX=csi)")
    assert "long" in text and str(EDGE + 3) in text and "a .bai cannot hold positions from 2^29 on" in text and "--csi" in text and "SVX_BUILD_INDEX=csi" in text
