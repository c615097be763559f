"""The host pieces of the sort's one-pass road, without a GPU: the stream reader of svision_amd/io/sam.py on an ``os.pipe()`` that a
thread feeds in writes of every size, the spool file over the BGZF writer with a zlib encoder and NumPy buffers (as
tests/test_sort_steps_cpu.py runs the writer), and the store of a pipe's records (sort.PipeStore) driven over crafted chunk sizes.
Expected values come from the text itself, gzip, svision_amd.io.bam and tests/htslike.py."""
import gzip
import os
import threading

import numpy as np
import pytest

from svision_amd import index, sort
from svision_amd.io import bam, sam
from tests import htslike, samtext
from tests.test_sort_steps_cpu import HostClock, host_clock, zlib_encode

REFS = [("chrA", 100_000), ("chrB", 50_000)]
HEADER = samtext.header_text(REFS).encode()


def _records(n=300):
    rng = np.random.default_rng(n)
    out = []
    for i in range(n):
        m = int(rng.integers(1, 400))
        out.append(dict(qname="read%d" % i, tid=int(rng.integers(0, 2)), pos=int(rng.integers(0, 40_000)), flag=0, mapq=60, cigar=[(m, "M")],
                        seq="".join("ACGT"[b] for b in rng.integers(0, 4, m)), qual=bytes(rng.integers(0, 40, m).astype(np.uint8)), tags=[("NM", "i", i)]))
    return out


RECORDS = _records()
BODY = b"".join(samtext.line(r, REFS) + b"\n" for r in RECORDS)


def _through_a_pipe(text, write, range_bytes, buffers=2):
    """``text`` written to a pipe ``write`` bytes a call by a thread -> (kind, header, [(chunk bytes, first line)], the reader)."""
    r, w = os.pipe()

    def feed():
        try:
            for at in range(0, len(text), write):
                os.write(w, text[at:at + write])
        except BrokenPipeError:
            pass
        finally:
            os.close(w)
    t = threading.Thread(target=feed, daemon=True)
    t.start()
    reader = sam.StreamReader(r, own=True)
    try:
        kind = sam.stream_kind(reader.peek())
        header = reader.header() if kind == sam.STREAM_SAM else b""
        chunks = [(bytes(memoryview(buf)[:n]), first) for buf, n, first in reader.chunks(range_bytes, header.count(b"\n"), buffers=buffers)] \
            if kind == sam.STREAM_SAM else []
    finally:
        reader.close()
    t.join(20)
    assert not t.is_alive()
    return kind, header, chunks, reader


def _check(text, header, chunks, range_bytes):
    """The header and the chunks cover the text once, in order; every chunk but the last ends behind a newline and is as long as
    range_bytes allows unless one line is longer; the line numbers count the lines in front."""
    closed = header if text.startswith(header) else header[:-1]          # (a header's last line without its newline is closed)
    assert closed + b"".join(c for c, _first in chunks) == text
    lines = header.count(b"\n")
    for k, (c, first) in enumerate(chunks):
        assert c and first == lines
        assert c.endswith(b"\n") or k == len(chunks) - 1
        assert len(c) <= range_bytes or c[:-1].count(b"\n") == 0, (len(c), range_bytes)
        lines += c.count(b"\n") + (not c.endswith(b"\n"))
    assert lines == text.count(b"\n") + (bool(text) and not text.endswith(b"\n"))


@pytest.mark.parametrize("range_bytes", [100, 4096, 1 << 16, sort.DEFAULT_SAM_CHUNK_BYTES])
@pytest.mark.parametrize("write", [1, 7, 1 << 16, 1 << 30], ids=["1", "7", "64K", "all"])
def test_chunks_cover_the_stream_once_whatever_the_reads_return(write, range_bytes):
    text = HEADER + (BODY[:20_000] if write == 1 else BODY)
    kind, header, chunks, reader = _through_a_pipe(text, write, range_bytes)
    assert kind == sam.STREAM_SAM and header == HEADER and reader.text_bytes == len(text)
    _check(text, header, chunks, range_bytes)
    longest = max(len(l) for l in text.split(b"\n")) + 1
    assert len(chunks) >= len(text) // max(range_bytes, longest)             # (no chunk is longer than range_bytes or one line)


def test_a_line_longer_than_the_chunk_grows_it():
    long_line = samtext.line(dict(RECORDS[0], qname="long", tags=[("XZ", "Z", "z" * 30_000)]), REFS) + b"\n"
    a, b = BODY.index(b"\n", 3000) + 1, BODY.index(b"\n", 9000) + 1
    text = HEADER + BODY[:a] + long_line + BODY[a:b] + long_line
    for write in (7, 1 << 30):
        _kind, header, chunks, _reader = _through_a_pipe(text, write, 1000)
        _check(text, header, chunks, 1000)
        assert sum(c == long_line for c, _first in chunks) == 2


def test_no_trailing_newline_is_a_line():
    text = HEADER + BODY[:-1]
    for range_bytes in (512, 1 << 20):
        _kind, header, chunks, _reader = _through_a_pipe(text, 1 << 16, range_bytes)
        _check(text, header, chunks, range_bytes)
        assert not chunks[-1][0].endswith(b"\n")


def test_header_only_and_header_at_a_read_boundary_and_headerless():
    for text in (HEADER, HEADER[:-1]):
        kind, header, chunks, _reader = _through_a_pipe(text, 5, 4096)
        assert kind == sam.STREAM_SAM and header == HEADER and chunks == []
    # the header's last line ends exactly where a read ends: the next read brings the first alignment line
    text = HEADER + BODY[:5000]
    kind, header, chunks, _reader = _through_a_pipe(text, len(HEADER), 4096)
    assert header == HEADER
    _check(text, header, chunks, 4096)
    kind, header, chunks, _reader = _through_a_pipe(BODY[:5000], 11, 700)          # no header at all
    assert kind == sam.STREAM_SAM and header == b""
    _check(BODY[:5000], header, chunks, 700)


class _ShortReads:
    """An object whose ``readinto`` returns at most ``most`` bytes a call, as a pipe does."""

    def __init__(self, data, most):
        self.data, self.at, self.most = data, 0, most

    def readinto(self, view):
        n = min(len(view), self.most, len(self.data) - self.at)
        view[:n] = self.data[self.at:self.at + n]
        self.at += n
        return n


BIG_HEADER = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:contig_%06d\tLN:%d\n" % (i, 1000 + i) for i in range(12000)) \
    + b"@PG\tID:aligner\tPN:aligner\n"


@pytest.mark.parametrize("most", [4096, 32768, 60000, 65536, 1 << 30], ids=["4K", "32K", "60000", "64K", "all"])
def test_a_header_larger_than_the_readers_steps(most):
    """A header of thousands of @SQ lines (above 128 KB) in reads below 64 KB, its end at every offset of a read: the header is the
    ``@`` lines and nothing else, and what lies behind it is the first chunk."""
    assert len(BIG_HEADER) > 2 * (128 << 10)
    body = BODY[:40_000]
    step = min(most, 60000)
    for cut in range(0, 40):                                    # the header shortened line by line: its end moves through a read
        head = BIG_HEADER if not cut else b"".join(BIG_HEADER.splitlines(True)[:-cut * 7])
        reader = sam.StreamReader(_ShortReads(head + body, most))
        assert sam.stream_kind(reader.peek()) == sam.STREAM_SAM
        assert reader.header() == head, (most, cut)
        chunks = [(bytes(memoryview(buf)[:n]), first) for buf, n, first in reader.chunks(1 << 20, head.count(b"\n"))]
        _check(head + body, head, chunks, 1 << 20)
    for pad in range(0, step, max(step // 97, 1)):               # ... and byte by byte: a comment line of every length in front of the end
        head = BIG_HEADER + b"@CO\t" + b"x" * pad + b"\n"
        reader = sam.StreamReader(_ShortReads(head + body, most))
        assert reader.header() == head, (most, pad)
        assert bytes(reader.buf) + reader.obj.data[reader.obj.at:] == body
    # a header line longer than many reads, and a last header line without its newline
    long_head = BIG_HEADER + b"@CO\t" + b"y" * 300_000 + b"\n"
    reader = sam.StreamReader(_ShortReads(long_head + body, most))
    assert reader.header() == long_head
    reader = sam.StreamReader(_ShortReads(long_head[:-1], most))
    assert reader.header() == long_head and not reader.buf


def test_a_line_of_many_reads_is_searched_once(monkeypatch):
    """A line far longer than the chunk: every byte of it is looked at once, not once a read."""
    looked = []
    real = sam._find_newline
    monkeypatch.setattr(sam, "_find_newline", lambda view, lo, hi, last=False: (looked.append(hi - lo), real(view, lo, hi, last))[1])
    line = samtext.line(dict(RECORDS[0], qname="long", tags=[("XZ", "Z", "z" * 400_000)]), REFS) + b"\n"
    text = HEADER + line + BODY[:5000]
    _kind, header, chunks, _reader = _through_a_pipe(text, 4096, 1000)
    _check(text, header, chunks, 1000)
    assert chunks[0][0] == line and sum(looked) < 3 * len(text)


def test_what_the_first_bytes_say():
    assert _through_a_pipe(b"", 1, 100)[0] == sam.STREAM_EMPTY
    assert _through_a_pipe(gzip.compress(HEADER + BODY), 1000, 100)[0] == sam.STREAM_GZIP
    raw = htslike._bgzf_block(sam.bam_header_bytes(sam.parse_header(HEADER)), 1) + htslike.EOF_BLOCK
    assert _through_a_pipe(raw, 1 << 16, 100)[0] == sam.STREAM_BAM
    assert _through_a_pipe(gzip.compress(b"BAM\x01" + bytes(100)), 3, 100)[0] == sam.STREAM_BAM
    assert _through_a_pipe(b"\x00\x01binary", 3, 100)[0] == sam.STREAM_OTHER
    assert sam.stream_kind(b"\x1f\x8b\x08\x00 not deflate at all") == sam.STREAM_BAM     # (the BAM road names what is broken)


def test_close_ends_a_reader_whose_writer_is_silent():
    """The reading thread never blocks in a read: a close while the writer holds the pipe open and writes nothing returns, and the
    descriptor is closed -- the writer's next write fails with EPIPE."""
    r, w = os.pipe()
    os.write(w, HEADER + BODY[:10_000])
    reader = sam.StreamReader(r, own=True)
    reader.header()
    gen = reader.chunks(1000, 0)
    next(gen)
    gen.close()
    with pytest.raises(BrokenPipeError):
        os.write(w, b"more")
    os.close(w)


def test_an_object_with_readinto():
    import io
    text = HEADER + BODY[:30_000]
    reader = sam.StreamReader(io.BytesIO(text))
    header = reader.header()
    chunks = [(bytes(memoryview(buf)[:n]), first) for buf, n, first in reader.chunks(2048, header.count(b"\n"))]
    _check(text, header, chunks, 2048)


# ---- the spool ----
def test_the_spool_is_an_unsorted_bam_of_the_records_in_arrival_order(tmp_path):
    head = sam.parse_header(HEADER)
    tid_of = sam.tid_table(head.references)
    recs = [sam.encode_line(samtext.line(r, REFS), tid_of) for r in RECORDS]
    header = sam.bam_header_bytes(head)
    out = str(tmp_path / "sorted.bam")
    spool = sort.Spool(out, header, zlib_encode, host_clock(), lambda b: np.frombuffer(b, np.uint8), "<stdin>")
    assert spool.path == "%s.spool.%d.bam" % (out, os.getpid())
    for chunk in (recs[:7], recs[7:250], recs[250:]):           # three chunks: less than a block, several blocks, the rest
        raw = b"".join(chunk)
        spool.put(np.frombuffer(raw + bytes(sort.STREAM_SLACK), np.uint8), len(raw), step=2 * sort.BLOCK)
    assert spool.finish() == spool.path and sorted(os.listdir(str(tmp_path))) == [os.path.basename(spool.path)]
    raw = open(spool.path, "rb").read()
    assert spool.bytes == len(raw) and raw[-28:] == htslike.EOF_BLOCK
    assert gzip.decompress(raw) == header + b"".join(recs)
    got = bam.read_bam_header(spool.path)
    assert got.references == head.references and list(got.lengths) == head.lengths and got.header_text.rstrip("\0") == head.text
    table = bam.read_bam(spool.path)
    assert len(table) == len(RECORDS)
    assert table.pos.tolist() == [r["pos"] for r in RECORDS] and table.tid.tolist() == [r["tid"] for r in RECORDS]
    members = list(index.bgzf_members(spool.path))                  # the project's own walk of the members: whole blocks of at most 0xFF00 bytes
    assert sum(isize for _at, _bsize, _xlen, isize in members) == len(header) + sum(len(r) for r in recs)
    assert max(isize for _at, _bsize, _xlen, isize in members) <= htslike.BLOCK
    spool.discard()
    assert os.listdir(str(tmp_path)) == []


def test_a_spool_that_fails_leaves_nothing(tmp_path):
    def refuse(buf, off):
        raise OSError("no space left")
    with pytest.raises(OSError):
        sort.Spool(str(tmp_path / "x.bam"), b"BAM\x01" + bytes(8), refuse, host_clock(), lambda b: np.frombuffer(b, np.uint8))
    assert os.listdir(str(tmp_path)) == []
    spool = sort.Spool(str(tmp_path / "x.bam"), b"BAM\x01" + bytes(8), zlib_encode, host_clock(), lambda b: np.frombuffer(b, np.uint8))
    spool.put(np.zeros(100 + sort.STREAM_SLACK, np.uint8), 100)
    spool.discard()                                             # (before finish: the temporary goes)
    assert os.listdir(str(tmp_path)) == []


def test_bam_bytes_are_copied_as_they_are(tmp_path):
    raw = htslike._bgzf_block(sam.bam_header_bytes(sam.parse_header(HEADER)), 1) + htslike._bgzf_block(bytes(70_000 % htslike.BLOCK), 1) + htslike.EOF_BLOCK
    r, w = os.pipe()
    t = threading.Thread(target=lambda: (os.write(w, raw), os.close(w)), daemon=True)
    t.start()
    reader = sam.StreamReader(r, own=True)
    assert sam.stream_kind(reader.peek()) == sam.STREAM_BAM
    path, n = sort.spool_copy(reader, str(tmp_path / "out.bam"), host_clock())
    reader.close()
    t.join(20)
    assert n == len(raw) and open(path, "rb").read() == raw and os.listdir(str(tmp_path)) == [os.path.basename(path)]


# ---- the growth rule ----
STORE_HEADER = sam.bam_header_bytes(sam.parse_header(HEADER))


def drive(chunks, budget, out):
    """sort.PipeStore itself over chunks of ``chunks`` bytes, chunk k filled with the byte value k % 251 + 1, as the key passes of a
    pipe drive it -- admit, buffer, keep per chunk, then the spool's finish or the join into the stream --, handed NumPy buffers and
    the zlib encoder -> (the store, the ledger's totals at every step with the record bytes seen and the chunk at that step, the
    joined stream or None).  A total is taken at every allocation's first use: when a buffer was kept, and at every copy of a join."""
    steps, at = [], {"seen": 0, "chunk": 0}
    store = sort.PipeStore(out, budget, 2 * sort.BLOCK, HostClock(), "<stdin>")

    def copy(dst, seg):
        steps.append((store.ledger.now, at["seen"], at["chunk"]))
        np.copyto(dst, seg)
    store.on(lambda: STORE_HEADER, lambda n_bytes: np.empty(n_bytes, np.uint8), copy, zlib_encode, lambda b: np.frombuffer(b, np.uint8))
    for k, c in enumerate(chunks):
        at["chunk"] = c
        store.admit(c)                                          # (a join for the spool is counted against the bytes seen before this chunk)
        at["seen"] += c
        buf = store.buffer(c)
        assert buf.size == c + (sort.STREAM_SLACK if store.spool is not None else 0) and not buf[c:].any()
        buf[:c] = k % 251 + 1
        store.keep(buf, c)
        del buf
        steps.append((store.ledger.now, at["seen"], c))
    store.finish()
    stream = None
    if store.mode == "in_core":
        stream = np.zeros(sum(chunks) + sort.STREAM_SLACK, np.uint8)
        store.fill(stream, 0)
    return store, steps, stream


def _chunk_bytes(chunks):
    return b"".join(bytes([k % 251 + 1]) * c for k, c in enumerate(chunks))


@pytest.mark.parametrize("chunks", [[100], [100] * 50, [1000, 10, 10, 5000, 36], [36] * 3 + [1 << 20], list(range(40, 4000, 37))],
                         ids=["one", "even", "mixed", "late_large", "rising"])
def test_the_growth_rule_keeps_both_conditions(chunks, tmp_path):
    total, out = sum(chunks), str(tmp_path / "sorted.bam")
    for budget in (1, chunks[0] - 1, chunks[0], 2 * chunks[0] + 3, 2 * chunks[0] + 4, total, 2 * total + 3, 2 * total + 4, 1 << 40):
        store, steps, stream = drive(chunks, budget, out)
        mode, ledger = store.mode, store.ledger
        assert mode == ("in_core" if 2 * total + sort.STREAM_SLACK <= budget else "spooled"), (budget, mode)
        for now, seen, chunk in steps:
            assert now <= budget or now == 0, (now, budget)                    # (a)
            assert now <= 2 * seen + chunk, (now, seen, chunk)                  # (b)
        assert ledger.peak == max(now for now, _seen, _chunk in steps)
        if mode == "in_core":
            assert ledger.peak == 2 * total + sort.STREAM_SLACK and ledger.grows == len(chunks) + 1
            assert stream[:total].tobytes() == _chunk_bytes(chunks) and not stream[total:].any() and ledger.now == stream.size
            assert store.spool_file is None and os.listdir(str(tmp_path)) == []
        else:
            assert store.spool_file == sort.spool_path(out) and store.spool_bytes == os.path.getsize(store.spool_file)
            assert gzip.decompress(open(store.spool_file, "rb").read()) == STORE_HEADER + _chunk_bytes(chunks)
        store.discard()
        assert os.listdir(str(tmp_path)) == []
    # a budget smaller than the first chunk spools at once: nothing was ever kept
    store, _steps, _stream = drive(chunks, chunks[0] // 2, out)
    assert store.mode == "spooled" and store.ledger.peak == 0
    store.discard()


def test_a_chunk_refused_mid_way_spools_the_kept_records_first(tmp_path):
    """Chunks of distinct byte values, a few hundred bytes each, and a budget that keeps the first three: the spool's inflated bytes are
    the header, then every chunk's bytes in arrival order -- the kept ones, joined, in front of the one that was refused."""
    chunks = [300, 410, 250, 520, 330, 280]
    budget = 2 * sum(chunks[:3]) + sort.STREAM_SLACK
    store, steps, stream = drive(chunks, budget, str(tmp_path / "sorted.bam"))
    assert store.mode == "spooled" and stream is None and not store.segments
    assert store.ledger.grows == 3 + 1 and store.ledger.peak == budget and store.ledger.now == 0     # three segments and their join for the spool
    assert gzip.decompress(open(store.spool_file, "rb").read()) == STORE_HEADER + _chunk_bytes(chunks)
    store.discard()
    assert os.listdir(str(tmp_path)) == []


def test_which_inputs_take_the_one_pass_road(tmp_path):
    regular, fifo = str(tmp_path / "a.sam"), str(tmp_path / "fifo")
    open(regular, "wb").write(HEADER)
    os.mkfifo(fifo)
    assert sort.is_stream("-") and sort.is_stream(fifo) and sort.is_stream(os.devnull)
    assert not sort.is_stream(regular) and not sort.is_stream(str(tmp_path / "missing"))
    assert "spool" in sort.STAGES


def test_the_svision_command_line_keeps_a_dash():
    from svision_amd import cli
    assert cli._bam_arg("-") == "-" and cli._bam_arg("x.bam") == os.path.abspath("x.bam")
    assert cli._input_list("-") is None and cli._input_list("-,-") is None
