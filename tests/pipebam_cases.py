"""The BAMs an aligner writes to a pipe, as the tests of the one-pass road take them (tests/test_pipe_bam_cpu.py, test_gpu_pipe_bam_call.py,
test_gpu_pipe_bam_sort.py): unsorted files of the test-side writer (tests/htslike.write_bam), a few hundred KB to a few MB each, written
once a session.  Every case names what it is there for:

  hifi           ~400 simulated reads of 2-15 kb (svision_amd.synth), blocks cut every 0xFF00 bytes at level 1 -- records and record
                 headers straddle blocks
  ont            reads of 100-200 kb: a record covers three blocks and more, so a range of 64 KB never completes one at first
  flush          a record that does not fit what is left of a block opens a new one (htslib's bgzf_flush_try), level 6
  stored         level 0: what ``samtools view -u`` and an uncompressed pipe give
  big_header     12,000 @SQ lines: the header alone fills many members
  one, none      a single record; a header and no record
  unmapped_tail  records without a reference (tid -1) among and behind the mapped ones
  cg             a record of more than 65,535 CIGAR operations: its CIGAR is in its CG:B:I tag
"""
import functools
import os
import struct
import tempfile
import threading
import zlib

import numpy as np

from tests import htslike, samtext

NAMES = ("hifi", "ont", "flush", "stored", "big_header", "one", "none", "unmapped_tail", "cg")
REFS = [("chrA", 900_000), ("chrB", 600_000)]
_DIR = []


def _dir():
    if not _DIR:
        _DIR.append(tempfile.TemporaryDirectory(prefix="pipebam_cases."))
    return _DIR[0].name


def _bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def _read(rng, i, refs, lo, hi, tid=None):
    """A read of lo..hi bases whose CIGAR consumes them all: clips, matches, an insertion and a deletion."""
    n = int(rng.integers(lo, hi + 1))
    tid = int(rng.integers(0, len(refs))) if tid is None else tid
    clip, ins = int(rng.integers(0, 40)), int(rng.integers(1, 60))
    m = n - clip - ins
    cigar = ([(clip, "S")] if clip else []) + [(m // 2, "M"), (ins, "I"), (int(rng.integers(1, 90)), "D"), (m - m // 2, "M")]
    unmapped = tid < 0
    return dict(qname="read%05d" % i, tid=tid, pos=-1 if unmapped else int(rng.integers(0, max(refs[tid][1] - 2 * n, 1))), flag=4 if unmapped else 0,
                mapq=0 if unmapped else 60, cigar=[] if unmapped else cigar, seq=_bases(rng, n), qual=bytes(rng.integers(0, 94, n, dtype=np.uint8)),
                tags=[("NM", "C", i % 200), ("RG", "Z", "rg1")])


def _hifi():
    from svision_amd import synth
    cfg = synth.SimConfig(contigs=list(REFS), coverage=2.5, read_len_mean=8_500.0, read_len_sd=3_000.0, seed=11)
    table, _genome, _svs = synth.simulate(cfg, with_genome=False, with_seq=True)
    rng = np.random.default_rng(11)
    recs = samtext.records_of_table(table, rng, tags=True)
    recs = [samtext.for_htslike(recs[i]) for i in rng.permutation(len(recs))]
    assert 300 < len(recs) < 600
    return list(zip(table.references, table.lengths)), recs, dict(level=1, policy="stream")


def _case(name):
    """-> (references, records in file order, write_bam's keywords)."""
    rng = np.random.default_rng(NAMES.index(name) + 100)
    if name == "hifi":
        return _hifi()
    if name == "ont":
        return REFS, [_read(rng, i, REFS, 100_000, 200_000) for i in range(9)], dict(level=1, policy="stream")
    if name == "flush":
        return REFS, [_read(rng, i, REFS, 200, 3_000) for i in range(400)], dict(level=6, policy="htslib")
    if name == "stored":
        return REFS, [_read(rng, i, REFS, 500, 6_000) for i in range(150)], dict(level=0, policy="stream")
    if name == "big_header":
        refs = [("contig%05d" % i, 10_000 + i) for i in range(12_000)]
        return refs, [_read(rng, i, refs, 300, 2_000) for i in range(120)], dict(level=6, policy="stream")
    if name == "one":
        return REFS, [_read(rng, 0, REFS, 5_000, 5_000)], dict(level=6, policy="stream")
    if name == "none":
        return REFS, [], dict(level=6, policy="stream")
    if name == "unmapped_tail":
        recs = [_read(rng, i, REFS, 300, 4_000, tid=-1 if i % 7 == 3 else None) for i in range(200)]
        return REFS, recs + [_read(rng, 200 + i, REFS, 300, 4_000, tid=-1) for i in range(40)], dict(level=1, policy="stream")
    assert name == "cg"
    recs = [_read(rng, i, REFS, 300, 4_000) for i in range(60)]
    cigar = [(1, "MIMD"[k % 4]) for k in range(70_001)]         # 1M 1I 1M 1D ... 1M: more operations than n_cigar_op holds
    n = htslike.query_len(cigar)
    recs.insert(30, dict(qname="long_cigar", tid=1, pos=1_000, flag=0, mapq=60, cigar=cigar, seq=_bases(rng, n), qual=None, tags=[("NM", "C", 1)]))
    return REFS, recs, dict(level=1, policy="stream")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(name, path: the BAM, data: its bytes, refs, recs, n, header: its header text): written once, left unchanged."""
    refs, recs, how = _case(name)
    path = os.path.join(_dir(), name + ".bam")
    header = samtext.header_text(refs)
    htslike.write_bam(path, refs, recs, header_text=header, index=False, **how)
    with open(path, "rb") as f:
        data = f.read()
    return dict(name=name, path=path, data=data, refs=refs, recs=recs, n=len(recs), header=header)


# ---- an independent reading of the stream: members by ``struct``, the records by zlib ----
def members(data):
    """The BGZF members of ``data`` -> [(offset, length)]; AssertionError where it is no chain of whole members."""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00", at
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert at + bsize <= len(data), at
        out.append((at, bsize))
        at += bsize
    return out


def inflate(data):
    """-> (the inflated bytes of the members of ``data``, where each one's start [members + 1])."""
    parts, dst = [], [0]
    for at, bsize in members(data):
        parts.append(zlib.decompress(data[at + 18:at + bsize - 8], -15))
        assert zlib.crc32(parts[-1]) == struct.unpack_from("<I", data, at + bsize - 8)[0]
        dst.append(dst[-1] + len(parts[-1]))
    return b"".join(parts), dst


@functools.lru_cache(maxsize=None)
def _record_bytes(name):
    return [htslike.encode_record(r) for r in case(name)["recs"]]


def record_bytes(c):
    """The case's records as the file holds them, in file order -> [bytes] (encoded once, left unchanged)."""
    return _record_bytes(c["name"])


class Fifo:
    """A FIFO in ``d`` that a daemon thread writes ``data`` into (the pattern of tests/test_gpu_sort_pipe.py): ``done()`` joins the writer
    and removes the FIFO, ``broke``: the reader closed before all was written."""

    def __init__(self, d, data, name="fifo"):
        self.path, self.broke = os.path.join(str(d), name), False
        os.mkfifo(self.path)

        def feed():
            try:
                with open(self.path, "wb") as f:
                    f.write(data)
            except BrokenPipeError:
                self.broke = True
        self.thread = threading.Thread(target=feed, daemon=True)
        self.thread.start()

    def done(self):
        self.thread.join(30)
        ended = not self.thread.is_alive()
        os.unlink(self.path)
        return ended
