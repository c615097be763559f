"""The host steps of svision_amd/sort.py without a GPU: the BGZF writer over a zlib encoder and a NumPy buffer, the record selection of
the pieces, the one reading of a file's members and header (svision_amd/index.py: bgzf_members, header_place) and the commit of the
pair of files.  Every expected value comes from zlib, gzip, struct and tests/htslike.py."""
import gzip
import os
import struct

import numpy as np
import pytest

from svision_amd import index, sort
from svision_amd.io import bai
from tests import htslike, sortcases
from tests import test_sort_spans_cpu as spancases

BLOCK = sort.BLOCK
assert BLOCK == htslike.BLOCK == 0xFF00


# ---- the writer ----
def zlib_encode(buf, off):
    members = [htslike._bgzf_block(bytes(buf[a:b]), 1) for a, b in zip(off[:-1], off[1:])]
    m = np.asarray([len(x) for x in members], np.int64)
    return np.frombuffer(b"".join(members), np.uint8), m, np.zeros(m.size, np.int64), np.zeros(0, np.int64)


def walk_members(raw):
    """-> (file offset of every member, the inflated offset of every block [members + 1]), by struct alone."""
    coff, dst, at = [], [0], 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 10:at + 16] == b"\x06\x00BC\x02\x00"
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        coff.append(at)
        dst.append(dst[-1] + struct.unpack_from("<I", raw, at + bsize - 4)[0])
        at += bsize
    assert at == len(raw)
    return coff, dst


def expected_voff(coff, dst, o):
    """The virtual offset of inflated offset ``o``: in the block whose bytes hold it, or offset 0 of the last block behind all."""
    for b in range(len(coff)):
        if dst[b] <= o < dst[b + 1]:
            return coff[b] << 16 | (o - dst[b])
    assert o == dst[-1]
    return coff[-1] << 16


def pieces_of(stream, mode):
    """The stream as sort_bam's pieces give it: (buffer, first, n_bytes) in chunks of one block, of two, or out of span buffers of two
    blocks that begin 13 bytes in front of their span (``first`` is not 0) and are given a block at a time."""
    n = stream.size
    if mode in ("one", "two"):
        step = BLOCK * (1 if mode == "one" else 2)
        for lo in range(0, n, step):
            yield stream, lo, min(lo + step, n) - lo
        return
    for s_lo in range(0, n, 2 * BLOCK):
        s_hi = min(s_lo + 2 * BLOCK, n)
        buf = np.concatenate([np.full(13, 0xEE, np.uint8), stream[s_lo:s_hi], np.full(4, 0xEE, np.uint8)])
        for lo in range(s_lo, s_hi, BLOCK):
            yield buf, 13 + lo - s_lo, min(lo + BLOCK, s_hi) - lo


def host_clock():
    return index._Clock(None, None, sort.STAGES)                # (the writer laps without device work: no torch is touched)


class HostClock(index._Clock):
    """The clock of a step whose buffers are NumPy arrays: no lap has device work to wait for."""

    def __init__(self):
        index._Clock.__init__(self, None, None, sort.STAGES)

    def lap(self, stage, device_work=True):
        index._Clock.lap(self, stage, False)


@pytest.mark.parametrize("mode", ["one", "two", "span"])
@pytest.mark.parametrize("n_stream", [0, 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7])
@pytest.mark.parametrize("n_head", [100, BLOCK, BLOCK + 1])
def test_writer_against_gzip_and_a_walk_of_its_members(tmp_path, n_head, n_stream, mode):
    rng = np.random.default_rng(n_head + n_stream)
    header, stream = rng.integers(0, 4, n_head, dtype=np.uint8), rng.integers(0, 7, n_stream, dtype=np.uint8)
    out = str(tmp_path / "out.bam")
    w = sort.BgzfWriter(out, zlib_encode, host_clock())
    w.put_header(header, n_head)
    n_put = 0
    for piece in pieces_of(stream, mode):
        w.put(*piece)
        n_put += 1
    written = w.finish()
    raw = open(w.tmp, "rb").read()
    w.discard()
    assert os.listdir(str(tmp_path)) == []
    assert gzip.decompress(raw) == header.tobytes() + stream.tobytes()
    assert raw[-28:] == htslike.EOF_BLOCK
    coff, dst = walk_members(raw)
    assert written.blocks == len(coff) == (n_head + BLOCK - 1) // BLOCK + (n_stream + BLOCK - 1) // BLOCK + 1
    assert written.coff.tolist() == coff and written.dst.tolist() == dst
    assert (written.chunks, written.stored_blocks, written.dynamic_blocks) == (n_put, 0, 0)
    assert (written.compressed_bytes, written.inflated_bytes) == (len(raw), n_head + n_stream)
    assert n_head in dst                                        # the first record opens a new block
    # record offsets in the stream: its first byte, a block's last and the next block's first, the stream's end
    offs = sorted({o for o in (0, min(BLOCK, n_stream) - 1, BLOCK, n_stream) if 0 <= o <= n_stream})
    got = bai.virtual_offsets(written.dst, written.coff, np.asarray(offs, np.uint64) + np.uint64(n_head))
    assert got.tolist() == [expected_voff(coff, dst, n_head + o) for o in offs]
    assert int(got[0]) & 0xFFFF == 0 and int(got[-1]) == (len(raw) - 28) << 16      # (the stream's end: the end-of-file block)


def test_writer_refuses_a_member_shorter_than_26_bytes(tmp_path):
    def short(buf, off):
        packed, m, stored, dynamic = zlib_encode(buf, off)
        m[-1] = 25
        return packed, m, stored, dynamic
    for in_header in (True, False):
        w = sort.BgzfWriter(str(tmp_path / "out.bam"), short if in_header else zlib_encode, host_clock(), source="in.bam")
        try:
            with pytest.raises(sort.SortWriteError, match="in.bam: svx_bgzf_deflate refused a block"):
                w.put_header(np.zeros(100, np.uint8), 100)      # (in_header: raises here)
                w.encode = short
                w.put(np.zeros(BLOCK + 5, np.uint8), 0, BLOCK + 5)
        finally:
            w.discard()                                         # the caller's cleanup (sort_bam's finally)
        assert os.listdir(str(tmp_path)) == []


def test_the_cut_is_one_function():
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7):
        want = [min(i * BLOCK, n) for i in range((n + BLOCK - 1) // BLOCK + 1)]
        assert sort.block_cuts(n).tolist() == want and sort.block_cuts(n, eof=True).tolist() == want + [n]
    assert sort.block_cuts(0).tolist() == [0] and sort.block_cuts(0, eof=True).tolist() == [0, 0]


# ---- the pieces ----
def _covers(chunks, total):
    at = 0
    for lo, hi in chunks:
        assert lo == at < hi
        at = hi
    assert at == total


@pytest.mark.parametrize("name", ["scaled", "ones", "one_long", "none", "all_empty"])
def test_chunks_cover_the_stream_once_and_one_rule_selects_their_records(name):
    lens = spancases._length_cases()[name]
    off = spancases._offsets(lens)
    total = int(off[-1])
    for step in (BLOCK, 2 * BLOCK, 1024 * BLOCK):
        chunks = list(sort.chunk_cuts(0, total, step))
        _covers(chunks, total)
        assert all(hi - lo == step for lo, hi in chunks[:-1])
        for budget in spancases._budgets(total):
            plan = sort.plan_spans(off, budget)
            _covers([c for sp in plan for c in sort.chunk_cuts(sp.lo, sp.hi, step)], total)
            for sp in plan:                                     # a span's chunks lie in its buffer, whole blocks but for the stream's last
                for lo, hi in sort.chunk_cuts(sp.lo, sp.hi, step):
                    assert sp.base <= lo and hi - sp.base + 4 <= sp.size and (lo % BLOCK == 0) and (hi % BLOCK == 0 or hi == total)
                assert tuple(int(v) for v in sort.records_touching(off, sp.lo, sp.hi)) == (sp.r_lo, sp.r_hi, sp.base)
        if not chunks:
            continue
        lo, hi = np.asarray(chunks, np.int64).T
        r_lo, r_hi, base = sort.records_touching(off, lo, hi)
        for i, (a, b) in enumerate(chunks):
            one = sort.records_touching(off, a, b)
            assert tuple(int(v) for v in one) == (int(r_lo[i]), int(r_hi[i]), int(base[i]))
            assert 0 <= r_lo[i] < r_hi[i] <= lens.size and base[i] == off[r_lo[i]] <= a and off[r_hi[i]] >= b


def test_in_core_selection_model_gives_the_gathered_stream():
    """The in-core generator over NumPy stand-ins: per chunk the selected records gathered into a buffer at their rebased offsets; the
    chunk's bytes in it, end to end, are the sorted stream."""
    rng = np.random.default_rng(8)
    lens = sortcases.segment_lengths() * 3
    off_in = spancases._offsets(lens)
    data = rng.integers(0, 256, int(off_in[-1]), dtype=np.uint8)
    for order in (rng.permutation(lens.size), np.arange(lens.size)):
        want, off_out = sortcases.gather_segments(data, off_in, order)
        off_out = np.asarray(off_out, np.int64)
        for step in (BLOCK, 3 * BLOCK):
            out = []
            for lo, hi in sort.chunk_cuts(0, int(off_out[-1]), step):
                r_lo, r_hi, base = (int(v) for v in sort.records_touching(off_out, lo, hi))
                buf = np.full(int(off_out[r_hi]) - base + 4, 0xA5, np.uint8)
                for r in range(r_lo, r_hi):
                    i = int(order[r])
                    buf[int(off_out[r]) - base:int(off_out[r + 1]) - base] = data[int(off_in[i]):int(off_in[i + 1])]
                out.append(buf[lo - base:hi - base])
            assert np.array_equal(np.concatenate(out), want)


# ---- members and header ----
REFS = [("chrA", 100_000), ("chrB", 50_000)]
RECORDS = [dict(tid=0, pos=10 * i, qname="r%d" % i, flag=0, mapq=30, cigar=[(20, "M")], seq="ACGTACGTACGTACGTACGT") for i in range(40)]


def _header_text(fill):
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
    return text + "@CO\t" + "x" * (fill - len(text) - 5) + "\n" if fill else text


def _dictionary_bytes():
    return 4 + sum(4 + len(name) + 1 + 4 for name, _ in REFS)


@pytest.fixture(scope="module")
def headers(tmp_path_factory):
    d = tmp_path_factory.mktemp("headers")
    cases = {"one_block": (_header_text(0), "htslib"), "three_blocks": (_header_text(2 * BLOCK + 999), "stream"),
             "fills_its_block": (_header_text(BLOCK - 8 - _dictionary_bytes()), "stream")}
    out = {}
    for name, (text, policy) in cases.items():
        path = str(d / (name + ".bam"))
        htslike.write_bam(path, REFS, RECORDS, level=1, policy=policy, header_text=text, index=False)
        out[name] = path
    return out


def _expected_place(raw):
    data = gzip.decompress(raw)
    l_text = struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, 8 + l_text)[0]
    at = 8 + l_text + 4
    for _ in range(n_ref):
        at += 4 + struct.unpack_from("<i", data, at)[0] + 4
    coff, dst = walk_members(raw)
    b = next(b for b in range(len(coff)) if dst[b] <= at < dst[b + 1])
    return (coff[b], at - dst[b], n_ref), data[:at], len(data)


@pytest.mark.parametrize("name", ["one_block", "three_blocks", "fills_its_block"])
def test_header_place_and_inflated_size(headers, name):
    path = headers[name]
    raw = open(path, "rb").read()
    place, head, n_inflated = _expected_place(raw)
    if name == "three_blocks":
        assert 2 * BLOCK < len(head) < 3 * BLOCK
    if name == "fills_its_block":
        assert len(head) == BLOCK and place[1] == 0
    got = index.header_place(path)
    assert tuple(got[:3]) == place == index.first_record(path) and got.head == head
    assert sort.inflated_size(path) == n_inflated
    # one pass: the members behind the header's, by the same generator, give the rest of the ISIZE sum
    members = index.bgzf_members(path)
    assert index.header_place(path, members).isize + sum(m[3] for m in members) == n_inflated
    assert [m[0] for m in index.bgzf_members(path)] == walk_members(raw)[0]
    new = sort.sorted_header_bytes(head)
    l_text, l_new = struct.unpack_from("<i", head, 4)[0], struct.unpack_from("<i", new, 4)[0]
    assert new[8:8 + l_new].startswith(b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrA") and new[8 + l_new:] == head[8 + l_text:]
    assert len(head) - 8 - l_text == _dictionary_bytes()


def test_members_refusals(headers, tmp_path):
    raw = open(headers["three_blocks"], "rb").read()
    coff, _dst = walk_members(raw)
    assert len(coff) >= 4 and raw[coff[1] + 12:coff[1] + 14] == b"BC"
    bad = {"cut_inside_a_member": raw[:coff[1] + 30],
           "no_bc_in_the_first": raw[:12] + b"XY" + raw[14:],
           "no_bc_in_the_second": raw[:coff[1] + 12] + b"XY" + raw[coff[1] + 14:],
           "bsize_below_its_header_and_footer": raw[:coff[1] + 16] + struct.pack("<H", 12 + 6 + 8 - 2) + raw[coff[1] + 18:]}
    for name, data in bad.items():
        p = str(tmp_path / (name + ".bam"))
        with open(p, "wb") as f:
            f.write(data)
        with pytest.raises(index.IndexBuildError, match="BGZF"):
            list(index.bgzf_members(p))
        with pytest.raises(sort.SortWriteError, match="BGZF"):
            sort.inflated_size(p)
        with pytest.raises(index.IndexBuildError, match="BGZF"):  # (the header lies in the first three members)
            index.first_record(p)
    p = str(tmp_path / "header_cut.bam")
    with open(p, "wb") as f:
        f.write(raw[:coff[2]])                                  # whole members, the header's last one missing
    with pytest.raises(index.IndexBuildError, match="BGZF"):
        index.header_place(p)


# ---- the commit ----
def _staged(tmp_path):
    out = str(tmp_path / "sorted.bam")
    f, tmp = index.temp_beside(out)
    with f:
        f.write(b"the sorted file")
    return out, tmp


@pytest.mark.parametrize("fail_at", [1, 2])
def test_commit_is_the_pair_or_nothing(tmp_path, monkeypatch, fail_at):
    out, tmp = _staged(tmp_path)
    real, calls = os.replace, []

    def replace(a, b):
        calls.append(b)
        if len(calls) == fail_at:
            raise OSError(28, "No space left on device")
        real(a, b)
    monkeypatch.setattr(os, "replace", replace)
    with pytest.raises(OSError):                                # (sort_bam wraps it: "writing ... failed")
        sort.commit_pair(tmp, out, b"the index")
    assert calls == [out, out + ".bai"][:fail_at] and os.listdir(str(tmp_path)) == []


def test_commit_modes_follow_the_umask(tmp_path):
    out, tmp = _staged(tmp_path)
    old = os.umask(0o027)
    try:
        sort.commit_pair(tmp, out, b"the index")
        index.write_into_place(str(tmp_path / "alone.bai"), b"an index")
    finally:
        os.umask(old)
    assert sorted(os.listdir(str(tmp_path))) == ["alone.bai", "sorted.bam", "sorted.bam.bai"]
    assert open(out, "rb").read() == b"the sorted file" and open(out + ".bai", "rb").read() == b"the index"
    assert all(os.stat(str(tmp_path / n)).st_mode & 0o777 == 0o640 for n in os.listdir(str(tmp_path)))


# ---- the join: the run's arrays and every input's own ----
def test_the_join_leaves_every_input_views_of_the_runs_offsets():
    """Three inputs of 3 + 0 + 2 records (the first in two ranges, the second a range that completed nothing) through sort._join with
    NumPy standing in for the device: the run's arrays are the inputs' end to end, and an input's pass holds no array of its own --
    its offsets are views into the run's, at its first record's number -- and nothing of what the join took."""
    from svision_amd import sort_sources
    lens = [[np.asarray([40, 50], np.int64), np.asarray([60], np.int64)], [], [np.asarray([70, 80], np.int64)]]
    records = [[2, 1], [0], [2]]
    kp, ranges, first, value = sort.RunPass(), 0, 0, 0
    for k, (own, n_recs) in enumerate(zip(lens, records)):
        part = sort_sources.InputPass(kp.seen)
        part.range_records, part.places, part.lens = list(n_recs), [(k, r) for r in range(len(n_recs))], own
        for l in own:
            v = np.arange(value, value + l.size, dtype=np.int32)
            part.host.append((v, v + 100, (v + 200).astype(np.uint16), v + 300))
            part.d_keys.append((v + 400, v + 500))
            value += l.size
        part.seen = int(sum(l.sum() for l in own))
        kp.parts.append(sort.Part(sort_sources.Opened("input%d" % k, None, None, None, None, None), part, ranges, first))
        kp.seen, ranges, first = kp.seen + part.seen, ranges + len(n_recs), first + sum(n_recs)
    dv = sort._Dev(None, None, None, None, HostClock())
    assert sort._join(dv, kp.parts[0].opened, kp, cat=np.concatenate, to_device=lambda a: a) is kp
    assert kp.n == 5 and kp.range_records == [2, 1, 0, 2] and kp.places == [(0, 0), (0, 1), (1, 0), (2, 0)]
    assert kp.off_in.tolist() == [0, 40, 90, 150, 220, 300] and kp.d_off_in is kp.off_in and kp.seen == 300
    for i, name in enumerate(("tid", "pos", "flag", "span", "d_tid", "d_pos")):
        assert getattr(kp, name).tolist() == [v + 100 * i for v in range(5)], name
    assert kp.flag.dtype == np.uint16
    for p, n, base in zip(kp.parts, (3, 0, 2), (0, 150, 150)):
        part = p.part
        assert part.n == n and part.base == base and (part.host, part.d_keys, part.lens) == ([], [], [])
        assert part.off_in.tolist() == kp.off_in[p.first_record:p.first_record + n + 1].tolist() and part.off_in[0] == base
        for own in (part.off_in, part.d_off_in):                # a view at the right record, not a copy
            assert own.base is kp.off_in and own.size == n + 1
            assert own.__array_interface__["data"][0] == kp.off_in.__array_interface__["data"][0] + 8 * p.first_record
    # no record at all: empty arrays of the right types, one offset
    empty = sort.RunPass()
    empty.parts.append(sort.Part(kp.parts[0].opened, sort_sources.InputPass(), 0, 0))
    sort._join(dv, kp.parts[0].opened, empty, cat=np.concatenate, to_device=lambda a: a)
    assert empty.n == 0 and empty.off_in.tolist() == [0] and empty.d_tid.dtype == np.int32 and empty.flag.dtype == np.uint16
    assert empty.parts[0].part.off_in.tolist() == [0]
