"""Inputs of the merge tests (tests/test_gpu_sort_merge.py): BAM files taken apart into their records' bytes and put together again under
other headers and other reference numberings.  Test-side only -- ``struct``, ``gzip`` and tests/htslike.py's BGZF block; no product code."""
import gzip
import struct

from tests import htslike


def raw_bam(path):
    """A BAM file -> (header text, [(reference, length)], [every record's bytes, block_size included])."""
    stream = gzip.decompress(open(path, "rb").read())
    assert stream[:4] == b"BAM\x01"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    text = stream[8:8 + l_text].rstrip(b"\0").decode("latin-1")
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", stream, at)[0]
        refs.append((stream[at + 4:at + 4 + l_name - 1].decode("latin-1"), struct.unpack_from("<i", stream, at + 4 + l_name)[0]))
        at += 8 + l_name
    records = []
    while at < len(stream):
        n = 4 + struct.unpack_from("<i", stream, at)[0]
        records.append(stream[at:at + n])
        at += n
    assert at == len(stream)
    return text, refs, records


def write_raw_bam(path, text, refs, records, level=1):
    """Header text, dictionary and record bytes -> an (unindexed) BAM whose blocks are cut every 0xFF00 bytes wherever that falls."""
    head = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode("latin-1") + struct.pack("<i", len(refs))
    for name, length in refs:
        head += struct.pack("<i", len(name) + 1) + name.encode("latin-1") + b"\0" + struct.pack("<i", length)
    stream = head + b"".join(records)
    with open(path, "wb") as f:
        for at in range(0, len(stream), htslike.BLOCK):
            f.write(htslike._bgzf_block(stream[at:at + htslike.BLOCK], level))
        f.write(htslike.EOF_BLOCK)
    return path


def tid(rec):
    return struct.unpack_from("<i", rec, 4)[0]


def pos(rec):
    return struct.unpack_from("<i", rec, 8)[0]


def flag(rec):
    return struct.unpack_from("<H", rec, 18)[0]


def next_tid(rec):
    return struct.unpack_from("<i", rec, 24)[0]


def qname(rec):
    return rec[36:36 + rec[12] - 1].decode()


def with_refs(rec, new_tid, new_next, next_pos=None):
    """The record with its refID and next_refID (and next_pos) set."""
    out = bytearray(rec)
    struct.pack_into("<i", out, 4, new_tid)
    struct.pack_into("<i", out, 24, new_next)
    if next_pos is not None:
        struct.pack_into("<i", out, 28, next_pos)
    return bytes(out)


def renumbered(rec, own, other):
    """The record of a file whose dictionary is ``own`` [(name, length)] as a file with the dictionary ``other`` stores it."""
    at = {name: i for i, (name, _n) in enumerate(other)}
    move = lambda v: v if v < 0 else at[own[v][0]]
    return with_refs(rec, move(tid(rec)), move(next_tid(rec)))


def unmapped(name):
    return htslike.encode_record(dict(tid=-1, pos=-1, qname=name, flag=4, mapq=0, cigar=[], seq="ACGTTGCA", qual=None, tags=[("NM", "C", 0)]))


def sq(refs):
    return "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
