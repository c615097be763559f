"""Crafted BAM record streams for the device ingest's record kernels (csrc/svx_bamdev.hip, svx_bamindex.hip: svx_bam_walk_*)
and a plain reference of what those kernels compute (tests/test_walkcases_cpu.py, tests/test_gpu_walk_kernels.py), and the
block table of tests/test_gpu_crc.py.  ``struct`` + NumPy only; no code of svision_amd/ is imported.

A case is a stream -- raw record bytes, the way the inflate leaves them in device memory -- and the ``starts`` of a walk:
byte offsets of record starts, ascending, the last entry the end of the part.  The reference follows SAMv1 4.2 (the record),
4.2.2 (a CIGAR of more than 65,535 operations lies in CG:B,I behind the placeholder ``<l_seq>S<span>N``) and 4.2.4 (the
widths of the optional fields' types); the status of a walk follows include/svx.h:

    0  the chain of block_size fields from start i ends exactly on start i + 1
    1  every record is well-formed measured against the end of the part, but the chain steps over start i + 1
       (what a stale index looks like)
    2  a record is malformed against the end of the part: block_size < 32, the record runs past the part's end (or less
       than a fixed-field block is left of the part), or the fixed fields + name + CIGAR + SEQ + QUAL exceed block_size
"""
import struct

import numpy as np

FILL = 0xA5                                                     # what the GPU tests pre-fill every output with
REFS = [("w0", 1 << 28), ("w1", 1 << 28), ("w2", 1 << 28)]
_LETTERS = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789/_", np.uint8)
_WIDTH = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
_SUB = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


# ---- the record builder ---------------------------------------------------------------------------------------------------
def aux_pad(n):
    """An optional field (XP:Z) of exactly ``n`` bytes: 0 or at least 4."""
    assert n == 0 or n >= 4
    return b"" if n == 0 else b"XPZ" + b"p" * (n - 4) + b"\x00"


def words_bytes(words):
    return struct.pack("<%dI" % len(words), *words)


def record(rng, l_read_name, n_cigar_op, l_seq, name=None, cigar=None, seq=None, qual=None, aux=b"", block_size=None, tid=None, pos=None,
           mapq=None, flag=None):
    """The raw bytes of one record, block_size included.  ``l_read_name`` / ``n_cigar_op`` / ``l_seq`` are what the fixed fields
    SAY; ``name`` / ``cigar`` / ``seq`` / ``qual`` (bytes) default to what they announce and may be anything for a hostile
    record, ``block_size`` defaults to the length of what follows it."""
    if name is None:
        name = _LETTERS[rng.integers(0, _LETTERS.size, l_read_name - 1)].tobytes() + b"\x00" if l_read_name else b""
    if cigar is None:
        w = (rng.integers(1, 1 << 20, n_cigar_op).astype(np.uint32) << 4 | rng.integers(0, 9, n_cigar_op).astype(np.uint32)).tolist()
        if n_cigar_op == 2:
            w[0] &= ~15                                          # (M: never the placeholder's S by accident)
        cigar = words_bytes(w)
    if seq is None:
        seq = rng.integers(0, 256, (l_seq + 1) // 2, dtype=np.uint8).tobytes()
    if qual is None:
        qual = b"\xff" * l_seq
    body = struct.pack("<iiBBHHHIiii", int(rng.integers(0, 3)) if tid is None else tid, int(rng.integers(0, 1 << 27)) if pos is None else pos,
                       l_read_name, int(rng.integers(0, 61)) if mapq is None else mapq, 4680, n_cigar_op,
                       int(rng.integers(0, 1 << 12)) if flag is None else flag, l_seq, -1, -1, 0) + name + cigar + seq + qual + aux
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


class Builder:
    """Records laid one behind the other, each -- where asked -- with its CIGAR words or its SEQ bytes at a chosen address modulo
    4 / 16 (the stream itself sits at a multiple of 16): the bytes that takes are optional-field bytes (aux_pad) added to the
    record in front of it, or, in front of the first record, bytes no record owns (the first start is not 0 then)."""

    def __init__(self, seed, lead=0):
        self.rng = np.random.default_rng(seed)
        self.buf = bytearray(lead)
        self.offsets = []
        self.seq_total = 0                                      # SEQ bytes so far = where the next record's bases go

    def _steer(self, at, want, mod):
        n = (want - (len(self.buf) + at)) % mod
        if n == 0:
            return
        if not self.offsets:
            self.buf += bytes(n)
            return
        while n < 4:
            n += mod
        o = self.offsets[-1]
        struct.pack_into("<I", self.buf, o, struct.unpack_from("<I", self.buf, o)[0] + n)
        self.buf += aux_pad(n)

    def add(self, l_read_name, n_cigar_op, l_seq, cig_mod4=None, seq_mod16=None, **kw):
        if cig_mod4 is not None:
            self._steer(36 + l_read_name, cig_mod4, 4)
        if seq_mod16 is not None:
            self._steer(36 + l_read_name + 4 * n_cigar_op, seq_mod16, 16)
        self.offsets.append(len(self.buf))
        self.buf += record(self.rng, l_read_name, n_cigar_op, l_seq, **kw)
        self.seq_total += (l_seq + 1) // 2

    def add_raw(self, data):
        self.offsets.append(len(self.buf))
        self.buf += data

    def add_cg(self, words, l_seq=0, front=b"", word_mod4=None, tag=None, back=b"", l_read_name=9):
        """A placeholder record ``<l_seq>S<span>N`` with ``front`` + a CG:B,I tag of ``words`` (or the bytes ``tag``) + ``back`` as
        its optional fields; ``word_mod4``: the tag's words at that address modulo 4 (an XP:Z field in front of ``front``)."""
        if tag is None:
            tag = b"CGBI" + struct.pack("<I", len(words)) + words_bytes(words)
        if word_mod4 is not None:
            at = len(self.buf) + 36 + l_read_name + 8 + (l_seq + 1) // 2 + l_seq + len(front) + 8
            n = (word_mod4 - at) % 4
            front = aux_pad(n + 4 if n else 0) + front
        self.add(l_read_name, 2, l_seq, cigar=words_bytes([l_seq << 4 | 4, 12345 << 4 | 3]), aux=front + tag + back)


class Case:
    def __init__(self, name, stream, starts, seq_dst=0, name_dst=0, host=True):
        self.name, self.stream, self.starts = name, bytes(stream), [int(s) for s in starts]
        self.seq_dst, self.name_dst = seq_dst, name_dst         # where the outputs begin, modulo 16 (the guard test's views)
        self.host = host                                        # well-formed for the host reader too (l_read_name >= 1)
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = walk_reference(self.stream, self.starts)
        return self._ref

    def __repr__(self):
        return self.name


# ---- the reference --------------------------------------------------------------------------------------------------------
def _fixed(stream, p):
    return struct.unpack_from("<IiiBBHHHI", stream, p)          # block_size, refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq


def _well_formed(stream, p, part_end):
    """The record at ``p`` against the end of the part -> its block_size, or None."""
    if p + 36 > part_end:
        return None
    bs, _tid, _pos, l_name, _mapq, _bin, n_cig, _flag, l_seq = _fixed(stream, p)
    if bs < 32 or p + 4 + bs > part_end or 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:     # (Python integers: no 32-bit wrap)
        return None
    return bs


def status_reference(stream, starts):
    out = []
    part_end = starts[-1]
    for p, end in zip(starts, starts[1:]):
        status = 0
        while p < end:
            bs = _well_formed(stream, p, part_end)
            if bs is None:
                status = 2
                break
            if p + 4 + bs > end:
                status = 1
                break
            p += 4 + bs
        if status == 0 and p != end:                            # (a start behind its successor: the chain is over it before its first step)
            status = 1
        out.append(status)
    return out


def cg_tag(stream, q, end):
    """The CG:B,I field among the optional fields [q, end) -> (offset of its words, their number), or None: the scan takes the
    widths of 4.2.4 and ends without a tag at an array that does not fit, at a type or an array subtype the spec does not
    know, and at the record's end."""
    while q + 3 <= end:
        tag, typ = stream[q:q + 2], chr(stream[q + 2])
        q += 3
        if typ == "B":
            if q + 5 > end:
                return None
            sub, n = chr(stream[q]), struct.unpack_from("<I", stream, q + 1)[0]
            if sub not in _SUB or end - (q + 5) < n * _SUB[sub]:
                return None
            if tag == b"CG" and sub == "I":
                return q + 5, n
            q += 5 + n * _SUB[sub]
        elif typ in "ZH":
            while q < end and stream[q]:
                q += 1
            q += 1
        elif typ in _WIDTH:
            q += _WIDTH[typ]
        else:
            return None
    return None


class Reference:
    pass


def walk_reference(stream, starts):
    """What the count pass and the extract pass owe for a walk: per start ``counts`` [n_starts, 4] (records, CIGAR words, QNAME
    bytes with one separator a record, status) and ``seq_bytes`` -- rows whose status is not 0 hold -1 --, per record of the
    status-0 intervals, in order, ``rec_off`` / ``tid`` / ``pos`` / ``flag`` / ``mapq`` / ``l_seq``, the offset arrays ``cig_off`` /
    ``name_off`` / ``seq_off`` (with their closing entries) into ``cigar`` / ``names`` ('\\n' behind each name) / ``seq``, and
    ``records`` (one dict each: where the record's parts lie in the stream)."""
    r = Reference()
    n_starts = len(starts) - 1
    status = status_reference(stream, starts)
    r.counts = np.full((n_starts, 4), -1, np.int64)
    r.seq_bytes = np.full(n_starts, -1, np.int64)
    r.counts[:, 3] = status
    r.records = []
    cigar, names, seq = [], [], []
    for i, (p, end) in enumerate(zip(starts, starts[1:])):
        if status[i]:
            continue
        n = words = name_bytes = bases = 0
        while p < end:
            bs, tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq = _fixed(stream, p)
            cig_at, n_words = p + 36 + l_name, n_cig
            seq_at = cig_at + 4 * n_cig                         # (behind the record's OWN words, placeholder or not)
            tagged = False
            if n_cig == 2:
                w0, w1 = struct.unpack_from("<II", stream, cig_at)
                if w0 == (l_seq << 4 | 4) and w1 & 15 == 3:
                    found = cg_tag(stream, seq_at + (l_seq + 1) // 2 + l_seq, p + 4 + bs)
                    if found is not None:
                        (cig_at, n_words), tagged = found, True
            nb = (l_seq + 1) // 2
            r.records.append(dict(off=p, tid=tid, pos=pos, flag=flag, mapq=mapq, l_seq=l_seq, l_read_name=l_name, n_cigar_op=n_cig, cig_at=cig_at,
                                  n_words=n_words, tagged=tagged, placeholder=n_cig == 2 and n_words == 2 and not tagged and w0 == (l_seq << 4 | 4) and w1 & 15 == 3,
                                  seq_at=seq_at, seq_bytes=nb))
            cigar.append(stream[cig_at:cig_at + 4 * n_words])
            names.append(stream[p + 36:p + 36 + max(l_name - 1, 0)] + b"\n")      # l_read_name counts the NUL; 0: an empty name
            seq.append(stream[seq_at:seq_at + nb])
            n, words, name_bytes, bases = n + 1, words + n_words, name_bytes + len(names[-1]), bases + nb
            p += 4 + bs
        r.counts[i, :3] = n, words, name_bytes
        r.seq_bytes[i] = bases
    rec = r.records
    r.rec_off = np.asarray([x["off"] for x in rec], np.uint64)
    r.tid, r.pos, r.l_seq = (np.asarray([x[f] for x in rec], np.int64).astype(np.uint32).view(np.int32) for f in ("tid", "pos", "l_seq"))
    r.flag, r.mapq = np.asarray([x["flag"] for x in rec], np.uint16), np.asarray([x["mapq"] for x in rec], np.uint8)
    r.cig_off = np.concatenate([[0], np.cumsum([x["n_words"] for x in rec])]).astype(np.int64)
    r.name_off = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.int64)
    r.seq_off = np.concatenate([[0], np.cumsum([x["seq_bytes"] for x in rec])]).astype(np.int64)
    r.cigar = np.frombuffer(b"".join(cigar), np.uint32)
    r.names = np.frombuffer(b"".join(names), np.uint8)
    r.seq = np.frombuffer(b"".join(seq), np.uint8)
    return r


def seq_geometry(src, dst, nbytes):
    """How a copy of ``nbytes`` SEQ bytes from address ``src`` to address ``dst`` (both modulo 16 is enough) splits into single
    bytes up to the destination's next multiple of 16 (head), whole 16-byte chunks, and single bytes behind them (tail);
    ``agree``: source and destination of the chunks agree modulo 16."""
    head = min((16 - dst % 16) % 16, nbytes)
    return dict(head=head, chunks=(nbytes - head) // 16, tail=(nbytes - head) % 16, short=nbytes < (16 - dst % 16) % 16, agree=(src + head) % 16 == (dst + head) % 16)


def facts(cases):
    """Which of the classes the kernels branch on a set of cases holds -- from the reference alone."""
    f = dict(n_starts=set(), l_read_name=set(), l_seq=set(), cigar=set(), chunks=set(), agree_chunks=set(), tails=set(), heads=set(), seq_pairs={},
             cigar_name_pairs=set(), cg_counts=set(), cg_mod4=set(), cg_with_bases=False, lookalikes=0, empty_middle=False, empty_last=False, all_empty=False,
             ends_with_bases=False, first_start_not_0=False)
    for c in cases:
        ref, n_starts = c.ref, len(c.starts) - 1
        if (ref.counts[:, 3] != 0).any():
            continue
        f["n_starts"].add(n_starts)
        empty = ref.counts[:, 0] == 0
        f["empty_middle"] |= bool(empty[:-1].any()) and not empty.all()
        f["empty_last"] |= bool(empty[-1]) and not empty.all()
        f["all_empty"] |= bool(empty.all()) and n_starts > 1
        f["first_start_not_0"] |= c.starts[0] != 0
        for k, x in enumerate(ref.records):
            f["l_read_name"].add(x["l_read_name"])
            f["l_seq"].add(x["l_seq"])
            if x["tagged"]:
                f["cg_counts"].add(x["n_words"])
                f["cg_mod4"].add(x["cig_at"] % 4)
                f["cg_with_bases"] |= x["l_seq"] > 0
            else:
                f["cigar"].add((x["n_words"], x["cig_at"] % 4))
            f["lookalikes"] += x["placeholder"]
            f["cigar_name_pairs"].add((x["cig_at"] % 4, (c.name_dst + int(ref.name_off[k])) % 4))
            if x["seq_bytes"]:
                src, dst = x["seq_at"] % 16, (c.seq_dst + int(ref.seq_off[k])) % 16
                g = seq_geometry(src, dst, x["seq_bytes"])
                f["seq_pairs"].setdefault((src, dst), set()).add("short" if g["short"] else g["chunks"])
                f["chunks"].add((g["chunks"], x["l_seq"] & 1))
                f["heads"].add(g["head"])
                if not g["short"]:
                    f["tails"].add(g["tail"])
                if g["agree"]:
                    f["agree_chunks"].add(g["chunks"])
        if ref.records:
            last = ref.records[-1]
            f["ends_with_bases"] |= last["l_seq"] > 0 and last["off"] + 4 + _fixed(c.stream, last["off"])[0] == len(c.stream)
    return f


# ---- the cases ------------------------------------------------------------------------------------------------------------
NAME_LENGTHS = (1, 2, 64, 65, 66, 129, 255)                    # (+ 0: the case "noname")
CIGAR_COUNTS = (0, 1, 63, 64, 65, 130, 1000)
SEQ_LENGTHS = (0, 1, 2, 3, 30, 31, 32, 33, 34)
CHUNK_COUNTS = (1, 63, 64, 65, 130)
CG_COUNTS = (0, 1, 63, 64, 65, 200)
N_STARTS = (1, 63, 64, 65, 130)


def _shape_stream():
    b = Builder(seed=11)
    rng = b.rng

    def filler(n):
        for _ in range(n):
            b.add(int(rng.integers(2, 40)), int(rng.integers(0, 20)), int(rng.integers(0, 100)))
    filler(20)
    for l in NAME_LENGTHS:
        b.add(l, 3, 10)
    filler(20)
    for n in CIGAR_COUNTS:
        for a in range(4):
            b.add(int(rng.integers(5, 30)), n, int(rng.integers(0, 40)), cig_mod4=a)
    filler(20)
    for l in SEQ_LENGTHS:
        b.add(8, 2, l)
    turn = 0
    for c in CHUNK_COUNTS:
        for odd in (0, 1):
            for agree in (False, True):
                # the bases go to seq_total: head bytes up to the next multiple of 16, c whole chunks, a tail
                head, tail = (16 - b.seq_total % 16) % 16, (5 * turn + 3) % 16
                nbytes = head + 16 * c + tail
                b.add(7, 1, 2 * nbytes - odd, seq_mod16=(b.seq_total + (0 if agree else 1 + (7 * turn) % 15)) % 16)
                turn += 1
        filler(3)
    filler(60)
    b.add(12, 4, 37)                                            # bases in the record that ends on the stream's last byte
    return b


def _spread(offsets, n):
    """``n`` of the offsets, the first among them, evenly."""
    return [offsets[i * len(offsets) // n] for i in range(n)]


def shape_cases():
    b = _shape_stream()
    end = len(b.buf)
    out = []
    for n in N_STARTS:
        if n == 1:
            starts = [b.offsets[0]]
        elif n == 130:                                          # 119 distinct starts, some of them two and three times (the first too), and the end twice
            d = _spread(b.offsets, 119)
            times = {0: 2, 40: 3, 60: 2, 61: 2, 80: 2, 100: 3, 110: 2, 118: 2}
            starts = [s for i, s in enumerate(d) for _ in range(times.get(i, 1))] + [end]          # (the last interval is empty)
            assert len(starts) == 130 and starts == sorted(starts)
        else:
            starts = _spread(b.offsets, n)
        out.append(Case("shape-%d" % n, b.buf, starts + [end]))
    out.append(Case("every-interval-empty", b.buf, [b.offsets[5]] * 4))
    # l_read_name 0: one separator and an empty name; the first start is not the stream's first byte
    b = Builder(seed=12, lead=7)
    for l_name, n_cig, l_seq in ((0, 3, 9), (5, 1, 0), (0, 0, 0), (17, 66, 40), (0, 70, 33), (3, 2, 5), (0, 1, 1)):
        b.add(l_name, n_cig, l_seq, cig_mod4=(l_seq + 1) % 4)
    out.append(Case("noname", b.buf, [b.offsets[0], b.offsets[3], len(b.buf)], host=False))
    return out


def cg_cases():
    """Placeholder records, their real CIGAR in CG:B,I -- small on purpose: nothing in the kernels asks for 65,536 operations."""
    b = Builder(seed=13)
    rng = b.rng

    def words(n):
        return (rng.integers(1, 1 << 24, n).astype(np.uint32) << 4 | rng.integers(0, 9, n).astype(np.uint32)).tolist()
    every = (b"XAAq" + b"Xcc\x85" + b"XCC\x85" + b"Xss\x01\x80" + b"XSS\x01\x80" + b"Xii\x01\x02\x03\x84" + b"XII\x01\x02\x03\x84" + b"Xff\x00\x00\x80\x3f"
             + b"XZZtext\x00" + b"XHH1AE3\x00" + b"".join(b"Y" + s.encode() + b"B" + s.encode() + struct.pack("<I", 3) + bytes(3 * _SUB[s]) for s in "cCsSiIf"))
    taken = []
    b.add(6, 5, 20)
    for i, n in enumerate(CG_COUNTS):
        b.add_cg(words(n), word_mod4=i % 4)
        taken.append(len(b.offsets) - 1)
    for a in range(4):
        b.add_cg(words(70 + a), word_mod4=a, front=b"NMi\x07\x00\x00\x00")
        taken.append(len(b.offsets) - 1)
    b.add_cg(words(9), front=every, back=b"NMi\x07\x00\x00\x00")                   # one field of every type in front of the tag
    taken.append(len(b.offsets) - 1)
    b.add_cg(words(80), l_seq=77, word_mod4=1)                 # with bases: SEQ behind the two placeholder words
    taken.append(len(b.offsets) - 1)
    b.add_cg(words(5), l_seq=6, front=b"XZZ\x00")
    taken.append(len(b.offsets) - 1)
    not_taken = len(b.offsets)
    b.add_cg(None, tag=b"CGBi" + struct.pack("<I", 4) + bytes(16))                  # signed: not the tag
    b.add_cg(words(4), front=b"XTBC" + struct.pack("<I", 1000))                     # an array that does not fit, in front of the tag
    b.add_cg(words(4), front=b"XQQ\x01\x02\x03\x04")                                # a type the spec does not know, in front of the tag
    b.add_cg(None, tag=b"CGBI" + struct.pack("<I", 50) + bytes(16))                 # the tag's own array does not fit
    b.add_cg(None, tag=b"", l_seq=4)                                                # the placeholder's shape, no optional field at all
    b.add_cg(None, tag=b"NMi\x07\x00\x00\x00" + b"XZZabc\x00")                      # ... and with fields, none of them CG
    b.add_cg(None, tag=b"CGZ12M\x00")                                               # CG of another type
    b.add(6, 2, 8)
    case = Case("cg", b.buf, [b.offsets[0], b.offsets[4], b.offsets[not_taken + 1], len(b.buf)])
    case.taken, case.not_taken = taken, list(range(not_taken, len(b.offsets) - 1))
    return [case]


def _good(rng):
    return record(rng, int(rng.integers(2, 30)), int(rng.integers(0, 12)), int(rng.integers(0, 60)))


def status_cases():
    """-> [(case, the interval that is bad, its status)]: six intervals of two good records each, one of them with a bad record
    between the two -- or, where the kind needs the part's end, as the last record of the last interval.  (None, None): a case
    of good intervals only."""
    rng = np.random.default_rng(14)
    good36 = record(rng, 1, 0, 0, name=b"\x00")                 # the smallest record: 36 bytes
    kinds = [("block_size-0", record(rng, 4, 1, 6, block_size=0), False),
             ("block_size-31", record(rng, 0, 0, 0, name=b"", aux=b"", block_size=31), False),
             ("l_seq-ffffffff", record(rng, 4, 1, 0xFFFFFFFF, seq=b"AB", qual=b"CD"), False),
             ("n_cigar-65535", record(rng, 4, 65535, 2, cigar=bytes(8)), False),
             ("fields-over-block_size", record(rng, 9, 3, 11, block_size=32 + 9 + 12 + 6 + 11 - 1), False),
             ("past-the-end", record(rng, 5, 2, 8, block_size=4000), True),
             ("35-bytes-left", good36[:35], True),
             ("3-bytes-left", good36[:3], True)]
    out = []
    for name, bad, last in kinds:
        buf, starts = bytearray(), []
        for i in range(6):
            starts.append(len(buf))
            buf += _good(rng)
            if i == (5 if last else 2):
                buf += bad                                      # (in the middle: its bytes end where the next good record begins)
                if last:
                    break
            buf += _good(rng)
        out.append((Case("status-" + name, buf, starts + [len(buf)], host=False), 5 if last else 2, 2))
    # a stale index: a start five bytes into a record, a start on the start of a record behind the next start
    b = Builder(seed=15)
    for _ in range(24):
        b.add(int(rng.integers(2, 30)), int(rng.integers(0, 12)), int(rng.integers(0, 60)))
    good = [b.offsets[3 * i] for i in range(8)] + [len(b.buf)]
    out.append((Case("status-good", b.buf, good), None, None))
    five = list(good)
    five[3] += 5
    out.append((Case("status-start-5-bytes-into-a-record", b.buf, five), 2, 1))
    later = list(good)
    later[3] = b.offsets[3 * 4 + 1]                             # behind start 4: interval 2 ends exactly there, interval 3 begins behind its own end
    out.append((Case("status-start-on-a-later-record", b.buf, later), 3, 1))
    return out


def guard_cases():
    """One record a launch.  All 16 x 16 (SEQ source address, destination address) pairs modulo 16, each with fewer bytes than
    the head (where the destination has a head), with 1 chunk + a tail and with 3 chunks + a tail -- the tails cover 0..15 --
    and all 4 x 4 (CIGAR source address, QNAME destination address) pairs modulo 4."""
    rng = np.random.default_rng(16)
    out = []

    def one(name, l_name, n_cig, l_seq, lead, seq_dst, name_dst):
        b = Builder(seed=int(rng.integers(1 << 30)), lead=lead)
        b.add(l_name, n_cig, l_seq)
        out.append(Case(name, b.buf, [lead, len(b.buf)], seq_dst=seq_dst, name_dst=name_dst))
    for src in range(16):
        for dst in range(16):
            head = (16 - dst) % 16
            for kind in range(3):
                if kind == 0 and head < 2:
                    continue                                    # no head (or a head of one byte: nothing shorter that has bases)
                tail = (src + 3 * dst + 7 * kind) % 16
                nbytes = int(rng.integers(1, head)) if kind == 0 else head + 16 * (1 if kind == 1 else 3) + tail
                l_name, n_cig = int(rng.integers(1, 20)), int(rng.integers(0, 6))
                one("guard-seq-%d-%d-%d" % (src, dst, kind), l_name, n_cig, 2 * nbytes - int(rng.integers(0, 2)),
                    (src - 36 - l_name - 4 * n_cig) % 16, dst, dst)
    for a in range(4):
        for d in range(4):
            l_name = int(rng.integers(60, 80))
            one("guard-cigar-%d-%d" % (a, d), l_name, 70, 5, (a - 36 - l_name) % 4, 4 * a + d, 4 * a + d)
    return out


def host_stream(case):
    """The case's records behind a BAM header: what tests/baicases.write_stream turns into a file the host reader takes."""
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
    head = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(REFS))
    for name, length in REFS:
        head += struct.pack("<i", len(name) + 1) + name.encode() + b"\x00" + struct.pack("<i", length)
    return head + case.stream[case.starts[0]:case.starts[-1]]


# ---- svx_bgzf_crc32: the block table (tests/test_gpu_crc.py) ----------------------------------------------------------------
CRC_SHORT = list(range(0, 301))
CRC_MIDDLE = list(range(4093, 4100)) + list(range(32765, 32772))
CRC_LONG = list(range(65230, 65537))


def _ordered(lengths, at):
    """``lengths`` in an order that, laid end to end from offset ``at``, brings every (offset mod 4, length mod 4) pair about as
    often as every other: the next block is always of the residue the current offset has seen least."""
    left = {r: sorted((v for v in lengths if v % 4 == r), reverse=True) for r in range(4)}
    seen, out = {}, []
    while any(left.values()):
        r = min((r for r in range(4) if left[r]), key=lambda r_: (seen.get((at % 4, r_), 0), r_))
        seen[(at % 4, r)] = seen.get((at % 4, r), 0) + 1
        v = left[r].pop()
        out.append(v)
        at += v
    return out


def crc_lengths():
    """The block lengths of the layout, in order: 0..300, 4093..4099, 32765..32771 and 65,230..65,536, every value once."""
    out = _ordered(CRC_SHORT, 0)
    out += CRC_MIDDLE
    return out + _ordered(CRC_LONG, sum(out))


def crc_classes(lengths, keep):
    """(dst_off mod 4, len mod 4) of the blocks whose length ``keep`` takes."""
    at, out = 0, set()
    for v in lengths:
        if keep(v):
            out.add((at % 4, v % 4))
        at += v
    return out
