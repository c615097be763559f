"""The host pieces of a BAM taken from a pipe in one pass, without a GPU: the member chunker and the header reader of
svision_amd/io/sam.py's StreamReader on an ``os.pipe()`` that a thread feeds in writes of every size, and the carrying of
svision_amd/index.py's stream_ranges with a zlib + ``struct`` model in the place of the device work.  Expected values come from the
stream itself through tests/pipebam_cases.py (members by ``struct``, records by tests/htslike.py) and from the file road's header
readers (io.bam.read_bam_header, index.first_record)."""
import io
import os
import struct
import threading
import time
import zlib

import numpy as np
import pytest

from svision_amd import index
from svision_amd.io import bam, sam
from tests import pipebam_cases as pb

WRITES = [1, 7, 4096, 65536, 1 << 30]
RANGES = [1, 100, 64 << 10, 1 << 20]


def _pipe(data, write):
    """``data`` written to a pipe ``write`` bytes a call by a thread -> (the reader, the thread)."""
    r, w = os.pipe()

    def feed():
        try:
            for at in range(0, len(data), write):
                os.write(w, data[at:at + write])
        except BrokenPipeError:
            pass
        finally:
            os.close(w)
    t = threading.Thread(target=feed, daemon=True)
    t.start()
    return sam.StreamReader(r, own=True), t


def _chunks(data, write, range_bytes):
    """-> [(the chunk's bytes, its stream offset)] of the whole stream, what peek() read first included."""
    reader, t = _pipe(data, write)
    try:
        assert sam.stream_kind(reader.peek()) == sam.STREAM_BAM
        out = [(bytes(memoryview(buf)[:n]), at) for buf, n, at in reader.member_chunks(range_bytes)]
    finally:
        reader.close()
    t.join(20)
    assert not t.is_alive() and reader.text_bytes == len(data)
    return out


def _prefix(data, limit):
    """The members of ``data`` that end within its first ``limit`` bytes."""
    return data[:max(at + n for at, n in pb.members(data) if at + n <= limit)]


# ---- the member chunker ----
@pytest.mark.parametrize("range_bytes", RANGES, ids=["1", "100", "64K", "1M"])
@pytest.mark.parametrize("write", WRITES, ids=["1", "7", "4K", "64K", "all"])
def test_member_chunks_cover_the_stream_once_whatever_the_reads_return(write, range_bytes):
    """big_header: 12,000 @SQ lines at level 6 make members of many lengths, so their boundaries fall all over a read (asserted
    below).  Writes of 1 and 7 bytes get a stream of their own -- a system call a byte for 600 KB would take the test's seconds --:
    the first 30,000 inflated bytes of that header as some 170 members of 61 to 300 bytes, a boundary at every offset of a write."""
    data = pb.case("big_header")["data"]
    if write < 4096:
        raw, cuts = pb.inflate(_prefix(data, 40_000))[0][:30_000], [0]
        while cuts[-1] < len(raw):
            cuts.append(min(cuts[-1] + 61 + 37 * len(cuts) % 240, len(raw)))
        data = b"".join(pb.htslike._bgzf_block(raw[a:b], 6) for a, b in zip(cuts, cuts[1:]))
    if write <= 7:
        assert {at % write for at, _n in pb.members(data)} == set(range(write))
    elif write < len(data):
        assert len({at % write for at, _n in pb.members(data)}) >= min(len(pb.members(data)) // 2, 20)
    chunks = _chunks(data, write, range_bytes)
    assert b"".join(c for c, _at in chunks) == data
    at = 0
    for c, said in chunks:
        assert c and said == at
        sizes = [n for _at, n in pb.members(c)]                 # (asserts that the chunk is whole members)
        # as many members as end within range_bytes, and at least one: a shorter chunk is followed by a member that would not fit
        assert len(c) <= range_bytes or len(sizes) == 1
        nxt = data[at + len(c):]
        assert not nxt or len(c) + pb.members(nxt)[0][1] > range_bytes
        at += len(c)


def test_every_case_in_chunks():
    for name in pb.NAMES:
        data = pb.case(name)["data"]
        for range_bytes in (64 << 10, 256 << 10):
            chunks = _chunks(data, 1 << 16, range_bytes)
            assert b"".join(c for c, _at in chunks) == data and all(pb.members(c) for c, _at in chunks)


def _refused(data, write=1 << 16, range_bytes=64 << 10):
    reader, t = _pipe(data, write)
    try:
        reader.peek()
        with pytest.raises(sam.BgzfStreamError) as exc:
            list(reader.member_chunks(range_bytes))
    finally:
        reader.close()
    t.join(20)
    assert not t.is_alive()
    return exc.value


def test_what_is_no_chain_of_bgzf_members_is_refused_with_its_offset():
    data = pb.case("flush")["data"]
    spans = pb.members(data)
    at, n = spans[5]
    # a stream cut inside a member: its header, its payload
    for cut in (at + 7, at + n - 3):
        exc = _refused(data[:cut])
        assert exc.offset == at and "offset %d" % at in str(exc) and "ends inside" in str(exc)
    # a plain gzip member (no BC field) behind five BGZF members
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    exc = _refused(data[:at] + co.compress(b"BAM\x01" + bytes(500)) + co.flush())
    assert exc.offset == at and "offset %d" % at in str(exc) and "plain gzip" in str(exc)
    # a BSIZE of 7
    bad = bytearray(data)
    struct.pack_into("<H", bad, at + 16, 7)
    exc = _refused(bytes(bad))
    assert exc.offset == at and "offset %d" % at in str(exc) and "BSIZE of 7" in str(exc)
    # the same through small reads and ranges: the offset does not depend on them
    assert _refused(bytes(bad), 7, 1).offset == at and _refused(data[:at + n - 3], 4096, 100).offset == at


def test_close_ends_a_member_reader_whose_writer_is_silent():
    """The thread polls: a close while the writer holds the pipe open in the middle of a member returns within the poll interval,
    and the descriptor is closed -- the writer's next write fails with EPIPE."""
    data = pb.case("flush")["data"]
    at, n = pb.members(data)[1]
    assert at + n // 2 < 1 << 16                                # (what a pipe holds: the write below does not block)
    r, w = os.pipe()
    os.write(w, data[:at + n // 2])
    reader = sam.StreamReader(r, own=True)
    gen = reader.member_chunks(at)
    buf, got, first = next(gen)                                 # the header's member, in front of the cut one
    assert (got, first) == (at, 0) and bytes(memoryview(buf)[:got]) == data[:at]
    t0 = time.perf_counter()
    gen.close()
    assert time.perf_counter() - t0 < 20 * sam.StreamReader.POLL_S
    with pytest.raises(BrokenPipeError):
        os.write(w, b"more")
    os.close(w)


# ---- the header ----
@pytest.mark.parametrize("name", pb.NAMES)
def test_the_stream_header_is_the_files(name):
    c = pb.case(name)
    want, first, place = bam.read_bam_header(c["path"]), index.first_record(c["path"]), index.header_place(c["path"])
    for write in (4096, 1 << 30):
        reader, t = _pipe(c["data"], write)
        try:
            assert sam.stream_kind(reader.peek()) == sam.STREAM_BAM
            got = reader.bam_header()
            assert got.first == first and got.head == place.head
            assert (got.table.references, got.table.lengths, got.table.header_text, got.table.sort_order, len(got.table)) == \
                (want.references, want.lengths, want.header_text, want.sort_order, 0)
            assert got.table.header_text == c["header"] and got.table.references == [r for r, _n in c["refs"]]
            # the members in front of the first record's are dropped, that one and all behind it stay for the chunks
            assert reader.buf_at == first[0]
            rest = b"".join(bytes(memoryview(buf)[:n]) for buf, n, _at in reader.member_chunks(64 << 10))
            assert rest == c["data"][first[0]:]
        finally:
            reader.close()
        t.join(20)
        assert not t.is_alive()


def test_a_header_that_is_cut_or_no_bam():
    c = pb.case("big_header")
    for data, words in ((c["data"][:pb.members(c["data"])[1][0]], "the BAM header is cut"), (c["data"][:pb.members(c["data"])[1][0] + 9], "no whole BGZF block"),
                        (pb.htslike._bgzf_block(b"SAM\x01" + bytes(100), 6), "not a BAM")):
        reader = sam.StreamReader(io.BytesIO(data))
        reader.peek()
        with pytest.raises(sam.BgzfStreamError, match=words):
            reader.bam_header()


# ---- stream_ranges over a model of the device work ----
class Model:
    """``work`` of index.stream_ranges by zlib and ``struct``: the range's blocks inflated, the records walked from ``entry``; every
    call is kept in ``calls`` as (stream offset of the range, its compressed bytes, entry, exit_off, total)."""

    def __init__(self):
        self.calls = []

    def __call__(self, pieces, blocks, entry):
        comp = b"".join(p.tobytes() for p in pieces)
        assert len(comp) == blocks.used and blocks.k == len(blocks.coff) == len(blocks.src_off)
        assert [n for _at, n in pb.members(comp)] == list(np.diff(np.append(blocks.coff, blocks.coff[0] + np.uint64(blocks.used))).astype(int))
        parts = []
        for k in range(blocks.k):
            at, n = int(blocks.src_off[k]), int(blocks.src_len[k])
            parts.append(zlib.decompress(comp[at:at + n], -15))
            assert len(parts[-1]) == int(blocks.isize[k])
        raw = b"".join(parts)
        rng = index.RecordRange()
        rng.blocks, rng.total, rng.records = blocks, len(raw), []
        rng.dst = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
        p = entry
        while p + 4 <= len(raw):
            size = 4 + struct.unpack_from("<i", raw, p)[0]
            if p + size > len(raw):
                break
            rng.records.append(raw[p:p + size])
            p += size
        rng.exit_off, rng.n_rec = p, len(rng.records)
        self.calls.append((int(blocks.coff[0]), comp, entry, p, len(raw)))
        return rng


def _ranges(data, range_bytes, stats=None):
    """The stream through bam_header, member_chunks and stream_ranges over the model -> (the ranges, the model, the chunks' sizes)."""
    reader = sam.StreamReader(io.BytesIO(data))
    reader.peek()
    got, model, sizes = reader.bam_header(), Model(), []

    def chunks():
        for item in reader.member_chunks(range_bytes):
            sizes.append(item[1])
            yield item
    try:
        return list(index.stream_ranges(chunks(), got.table, got.first, work=model, name="the pipe", stats=stats)), model, sizes
    finally:
        reader.close()


def _largest_record_blocks(c):
    """The compressed bytes of the members that hold the record which spans the most of them."""
    spans = pb.members(c["data"])
    _raw, dst = pb.inflate(c["data"])
    ends = np.cumsum([0] + [sz for _at, sz in spans])
    at, best = index.first_record(c["path"])[:2], 0
    p = dst[[a for a, _n in spans].index(at[0])] + at[1]
    for rec in pb.record_bytes(c):
        lo, hi = np.searchsorted(dst, p, "right") - 1, np.searchsorted(dst, p + len(rec), "left")
        best, p = max(best, int(ends[hi] - ends[lo])), p + len(rec)
    return best


@pytest.mark.parametrize("range_bytes", [1, 64 << 10, 256 << 10, 1 << 30], ids=["1", "64K", "256K", "whole"])
@pytest.mark.parametrize("name", pb.NAMES)
def test_every_record_completes_in_one_range_in_order(name, range_bytes):
    c = pb.case(name)
    data, stats = c["data"], {}
    ranges, model, sizes = _ranges(data, range_bytes, stats)
    # every record once, in stream order, and the last range says that it is the last
    assert [r for rng in ranges for r in rng.records] == pb.record_bytes(c)
    assert [rng.at_end for rng in ranges] == [False] * (len(ranges) - 1) + [True]
    assert all(rng.n_rec for rng in ranges) or c["n"] == 0 or range_bytes == 1       # (a range of one member: the end-of-file marker's is empty)
    # the chain entry -> exit_off is unbroken over every call of the work, in the stream's inflated bytes
    _raw, dst = pb.inflate(data)
    abs_of = dict(zip([at for at, _n in pb.members(data)], dst))
    first = index.first_record(c["path"])
    at = abs_of[first[0]] + first[1]
    for k, (coff, comp, entry, exit_off, total) in enumerate(model.calls):
        assert abs_of[coff] + entry == at and data[coff:coff + len(comp)] == comp
        at = abs_of[coff] + exit_off
        if exit_off == entry and exit_off < total:              # none completes: the next call has these bytes and more, from the same entry
            nxt = model.calls[k + 1]
            assert nxt[0] == coff and nxt[2] == entry and len(nxt[1]) > len(comp)
    assert at == dst[-1] and model.calls[-1][0] + len(model.calls[-1][1]) == len(data)
    assert [rng.place for rng in ranges] == [(coff, len(comp), entry) for coff, comp, entry, exit_off, total in model.calls if exit_off != entry or exit_off == total]
    # host memory: one chunk and one carried record's blocks
    blocks = _largest_record_blocks(c) if c["n"] else 0
    assert stats["held_peak"] == max(len(comp) for _c, comp, _e, _x, _t in model.calls) <= max(sizes) + blocks and stats["carry_peak"] <= blocks
    assert stats["ranges"] == len(model.calls) == len(sizes) and stats["grown"] == len(model.calls) - len(ranges)


def test_a_range_in_which_no_record_completes_grows():
    stats = {}
    ranges, model, sizes = _ranges(pb.case("ont")["data"], 64 << 10, stats)
    assert stats["grown"] >= 2 * len(ranges) and max(sizes) <= 1 << 16
    assert max(rng.place[1] for rng in ranges) > 3 << 16        # a record of three blocks and more: its range grew that far


def test_a_stream_cut_inside_a_record():
    c = pb.case("hifi")
    spans = pb.members(c["data"])
    cut = spans[len(spans) // 2][0]                             # a member boundary in the middle: records straddle every one
    for data in (c["data"][:cut], c["data"][:cut] + pb.htslike.EOF_BLOCK):
        for range_bytes in (64 << 10, 1 << 30):
            with pytest.raises(index.IndexBuildError, match=r"^the pipe is cut inside a record: its last record starts \d+ bytes before the end of "
                                                            r"the data and does not fit$"):
                _ranges(data, range_bytes)
    with pytest.raises(index.IndexBuildError, match=r"^the pipe: no whole BGZF block at stream offset %d" % cut):
        _ranges(c["data"][:cut + 100], 64 << 10)
