"""The oracle and the files of the index-build tests (tests/test_bai_cpu.py, tests/test_gpu_bai_build.py).  Shares no code with
svision_amd/io/bai.py or svision_amd/index.py: ``walk`` inflates every BGZF block with zlib and follows the chain of block_size
fields from the header's end with struct; tests/htslike.write_bai turns the walked records into the expected index."""
import bisect
import struct
import zlib

import numpy as np

from tests import htslike

REFS = [("chrA", 400_000), ("chrEmpty", 50_000), ("chrB", 300_000)]
BLOCK = htslike.BLOCK
NO_START = 0xFFFFFFFFFFFFFFFF


class Walked:
    """A BAM as the oracle sees it: ``coff`` / ``dst`` per BGZF block (file offset, offset of its bytes in ``stream``; ``dst`` has a
    closing entry), ``header_end``, per record ``offsets`` and ``records`` (dicts for htslike.write_bai), the records' virtual
    offsets + the end's (``voffs``) and per block the first record start (``first``, NO_START where none)."""

    def block_of(self, off):                                    # exactly behind a block's last byte: the next block that holds data (or the last)
        return bisect.bisect_right(self.dst[:-1], off) - 1

    def voff(self, off):
        b = self.block_of(off)
        return self.coff[b] << 16 | (off - self.dst[b])


def bgzf_blocks(raw):
    """-> [(file offset, inflated bytes)] of every BGZF block of ``raw``."""
    out, at = [], 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", raw, at + 10)[0]
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        data = zlib.decompress(raw[at + 12 + xlen:at + bsize - 8], -15)
        assert zlib.crc32(data) & 0xFFFFFFFF == struct.unpack_from("<I", raw, at + bsize - 8)[0]
        out.append((at, data))
        at += bsize
    return out


def _cg_words(aux):
    """The words of a CG:B,I tag among the optional fields ``aux``, or None."""
    width = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    p = 0
    while p + 3 <= len(aux):
        tag, typ = aux[p:p + 2], chr(aux[p + 2])
        p += 3
        if typ == "B":
            sub, n = chr(aux[p]), struct.unpack_from("<i", aux, p + 1)[0]
            p += 5
            if tag == b"CG" and sub == "I":
                return struct.unpack_from("<%dI" % n, aux, p)
            p += n * width[sub]
        elif typ in "ZH":
            p = aux.index(b"\x00", p) + 1
        else:
            p += width[typ]
    return None


def walk(path):
    w = Walked()
    blocks = bgzf_blocks(open(path, "rb").read())
    w.coff = [c for c, _d in blocks]
    w.dst = [0]
    for _c, d in blocks:
        w.dst.append(w.dst[-1] + len(d))
    s = w.stream = b"".join(d for _c, d in blocks)
    assert s[:4] == b"BAM\x01"
    p = 8 + struct.unpack_from("<i", s, 4)[0]
    n_ref = struct.unpack_from("<i", s, p)[0]
    p += 4
    w.references = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", s, p)[0]
        w.references.append((s[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from("<i", s, p + 4 + l_name)[0]))
        p += 8 + l_name
    w.header_end, w.offsets, w.records = p, [], []
    while p < len(s):
        size, tid, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", s, p)
        assert size >= 32 and p + 4 + size <= len(s)
        at = p + 36 + l_name
        words = struct.unpack_from("<%dI" % n_cig, s, at)
        if n_cig == 2 and words[0] == (l_seq << 4 | 4) and words[1] & 15 == 3:
            real = _cg_words(s[at + 8 + (l_seq + 1) // 2 + l_seq:p + 4 + size])
            words = real if real is not None else words
        w.offsets.append(p)
        w.records.append({"tid": tid, "pos": pos, "flag": flag, "cigar": [(x >> 4, htslike.OPS[x & 15]) for x in words]})
        p += 4 + size
    assert p == len(s)
    w.voffs = [w.voff(o) for o in w.offsets] + [w.voff(len(s))]
    w.first = [NO_START] * len(blocks)
    for o in reversed(w.offsets):
        w.first[w.block_of(o)] = o
    return w


def expected_bai(tmp_dir, walked):
    """htslike's index of the walked records, as bytes."""
    path = str(tmp_dir / "expected.bai")
    htslike.write_bai(path, walked.references, walked.records, walked.voffs)
    return open(path, "rb").read()


def arrays(walked):
    """The walked records as the arguments of svision_amd.io.bai.bai_bytes."""
    r = walked.records
    pos = np.asarray([x["pos"] for x in r], np.int64)
    end = pos + np.asarray([htslike.ref_len(x["cigar"]) or 1 for x in r], np.int64)
    return (len(walked.references), np.asarray([x["tid"] for x in r], np.int64), pos, end, np.asarray([x["flag"] for x in r], np.int64),
            np.asarray(walked.voffs[:-1], np.uint64), np.asarray(walked.voffs[1:], np.uint64))


# ---- the files ------------------------------------------------------------------------------------------------------------
def _bases(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def short_records(seed=1, n=300, read=2600, cg=False):
    """``n`` reads of about ``read`` bases with bases and qualities on chrA and chrB (chrEmpty has none), among them placed
    unmapped reads (flag 4 with a reference), secondary and supplementary ones, a tail of reads without a reference and,
    ``cg``, one alignment of more than 65,535 operations (its real CIGAR in the CG tag)."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        tid = 0 if i < n * 3 // 5 else 2
        length = REFS[tid][1]
        l = int(rng.integers(read // 2, read * 3 // 2))
        pos = int(rng.integers(0, length - 2 * l))
        if i % 17 == 5:                                         # a placed unmapped read: its mate's reference and position, no CIGAR
            recs.append(dict(tid=tid, pos=pos, qname="u%d" % i, flag=4 | 1 | 64, mapq=0, cigar=[], seq=_bases(rng, 200), qual=bytes(rng.integers(2, 40, 200, dtype=np.uint8)),
                             next_tid=tid, next_pos=pos, tags=[("RG", "Z", "rg1")]))
            continue
        d, ins = int(rng.integers(30, 400)), int(rng.integers(30, 200))
        a = l // 3
        cigar = [(17, "S"), (a, "M"), (d, "D"), (a, "M"), (ins, "I"), (l - 2 * a - ins - 17, "M")]
        recs.append(dict(tid=tid, pos=pos, qname="read/%d/ccs" % i, flag=(0, 16, 256, 2048)[i % 4], mapq=int(rng.integers(0, 61)), cigar=cigar, seq=_bases(rng, l),
                         qual=bytes(rng.integers(2, 41, l, dtype=np.uint8)), tags=[("NM", "i", d + ins), ("RG", "Z", "rg2"), ("qs", "Bs", [1, -2, 3])]))
    if cg:
        ops = [(1, "M"), (1, "I")] * 33_500 + [(40, "M")]
        recs.append(dict(tid=0, pos=120_000, qname="long_cigar", flag=0, mapq=60, cigar=ops, seq="*", tags=[("NM", "i", 7)]))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    for i in range(9):                                          # the tail: no reference, no position
        recs.append(dict(tid=-1, pos=-1, qname="nowhere%d" % i, flag=4, mapq=0, cigar=[], seq=_bases(rng, 300), qual=bytes(rng.integers(2, 40, 300, dtype=np.uint8))))
    return recs


def long_records(seed=2):
    """Fourteen reads of 100-200 kb with bases and qualities among two hundred short ones without bases: most blocks of the file
    lie inside one record."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(14):
        tid = 0 if i < 8 else 2
        l = int(rng.integers(100_000, 200_000))
        span = min(l, REFS[tid][1] // 3)
        pos = int(rng.integers(0, REFS[tid][1] - span - 10))
        recs.append(dict(tid=tid, pos=pos, qname="ont/%d" % i, flag=0, mapq=60, cigar=[(l - span, "S"), (span, "M")] if l > span else [(l, "M")], seq=_bases(rng, l),
                         qual=bytes(rng.integers(2, 41, l, dtype=np.uint8)), tags=[("NM", "i", i)]))
    for i in range(200):
        tid = 0 if i < 120 else 2
        recs.append(dict(tid=tid, pos=int(rng.integers(0, REFS[tid][1] - 5000)), qname="s%d" % i, flag=16 * (i & 1), mapq=30, cigar=[(int(rng.integers(500, 4000)), "M")],
                         seq="*", tags=[("XP", "Z", "")]))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return recs


def _pad_to(path, recs, k, target_of, want):
    """Write ``recs`` (streamed policy) with the XP:Z tag of record ``k`` grown until ``target_of(walk)`` -- a byte offset of the
    inflated stream behind that tag -- is ``want`` modulo the block size.  Every byte added moves the target by one."""
    htslike.write_bam(path, REFS, recs, level=1, policy="stream", index=False)
    at = target_of(walk(path))
    tags = [list(t) for t in recs[k]["tags"]]
    xp = next(t for t in tags if t[0] == "XP")
    xp[2] = xp[2] + "p" * ((want - at) % BLOCK)
    recs[k] = dict(recs[k], tags=[tuple(t) for t in tags])
    htslike.write_bam(path, REFS, recs, level=1, policy="stream", index=False)
    return walk(path)


def write_long(path):
    """long_records under the streamed policy, one short record padded so that the block_size field of the record behind it
    straddles a block boundary (its first two bytes end one block, the other two open the next).  -> (walk, that record's index)"""
    recs = long_records()
    k = next(i for i, r in enumerate(recs) if r["seq"] == "*" and i > 40)
    w = _pad_to(path, recs, k, lambda w_: w_.offsets[k + 1], BLOCK - 2)
    return w, k + 1


def decoy_copy():
    """The exact bytes of two encoded records that no file holds as records."""
    return b"".join(htslike.encode_record(dict(tid=t, pos=p, qname=q, flag=0, mapq=50, cigar=[(120, "M")], seq="ACGT" * 30, qual=bytes([30] * 120), tags=[("NM", "i", 1)]))
                    for t, p, q in ((0, 1234, "decoy/1"), (2, 77, "decoy/2")))


def write_decoy(path):
    """short_records under the streamed policy, one record carrying decoy_copy() in a B,C array that begins on the first byte of a
    BGZF block (XP:Z in front of it is the padding).  -> (walk, offset of the copy in the inflated stream)"""
    recs = short_records(seed=5, n=200)
    copy = decoy_copy()
    k = next(i for i, r in enumerate(recs) if r["tid"] == 0 and r["cigar"] and i > 30)
    recs[k] = dict(recs[k], tags=[("XP", "Z", "p" * 40_000), ("XD", "BC", list(copy))])
    w = _pad_to(path, recs, k, lambda w_: w_.stream.index(copy), 0)
    return w, w.stream.index(copy)


def write_stream(path, stream, level=1):
    """An inflated BAM stream as BGZF blocks cut every 0xFF00 bytes + the EOF block."""
    with open(path, "wb") as f:
        for at in range(0, len(stream), BLOCK):
            f.write(htslike._bgzf_block(stream[at:at + BLOCK], level))
        f.write(htslike.EOF_BLOCK)
