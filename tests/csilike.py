"""A CSI writer, parser and region query that share NO code with svision_amd/io/csi.py: a second reading of the CSIv1 layout,
``struct`` + ``zlib`` and plain loops, in the spirit of tests/htslike.py (whose record dicts and ``ref_len`` it takes).

  payload(...)          the index of a coordinate-sorted record list, in the project's own style -- loffset = the linear index, empty
                        windows filled from the right, at the bin's first window -- or ``foreign=True``, what other writers leave:
                        loffsets from a linear index filled from the LEFT (lower bounds only), every third one 0, a bin's chunks merged
                        where one ends in the BGZF block the next begins in, no pseudo-bin on one reference, no n_no_coor, 28 aux bytes
  parse(payload)        the inflated bytes -> a dict
  query(idx, ...)       what a reader does for a region: the bins that overlap it, the loffset of the lowest existing bin that holds the
                        region's start (else of its parents, else 0), the chunks whose end lies behind that offset
  reached / brute       the records a reader gets through those chunks and keeps / the records that overlap the region

The equality the tests ask is reached == brute: nobody here can compare bytes with htslib's."""
import struct
import zlib

from tests import htslike

EOF_BLOCK = htslike.EOF_BLOCK
AUX = bytes(range(1, 29))                                       # 28 bytes a foreign writer left (tabix keeps its configuration there)


def first_of(level):
    return ((1 << 3 * level) - 1) // 7


def reg2bin(beg, end, min_shift, depth):
    end -= 1
    shift, level = min_shift, depth
    while level > 0:
        if beg >> shift == end >> shift:
            return first_of(level) + (beg >> shift)
        shift += 3
        level -= 1
    return 0


def reg2bins(beg, end, min_shift, depth):
    end -= 1
    out, shift = [], min_shift + 3 * depth
    for level in range(depth + 1):
        out += range(first_of(level) + (beg >> shift), first_of(level) + (end >> shift) + 1)
        shift -= 3
    return out


def bin_start_window(b, depth):
    """The first smallest-level window of bin ``b``."""
    level = 0
    while first_of(level + 1) <= b:
        level += 1
    return (b - first_of(level)) << 3 * (depth - level)


def parent(b):
    return (b - 1) >> 3


def span_of(rec):
    beg = rec["pos"]
    return beg, beg + (htslike.ref_len(rec.get("cigar", [])) or 1)


def depth_for(longest, min_shift):
    d = 0
    while 2 ** (min_shift + 3 * d) < longest + 256:
        d += 1
    return d


def payload(references, records, voffs, min_shift=14, depth=None, foreign=False):
    n_ref = len(references)
    if depth is None:
        depth = depth_for(max([l for _n, l in references] + [0]), min_shift)
    bins = [dict() for _ in range(n_ref)]                       # bin -> [[beg, end]] in file order
    linear = [dict() for _ in range(n_ref)]
    meta = [[None, None, 0, 0] for _ in range(n_ref)]
    n_no_coor, last = 0, None
    for i, rec in enumerate(records):
        tid = rec["tid"]
        if tid < 0:
            n_no_coor += 1
            continue
        beg, end = span_of(rec)
        b = reg2bin(beg, end, min_shift, depth)
        if last != (tid, b):
            bins[tid].setdefault(b, []).append([voffs[i], voffs[i + 1]])
            last = (tid, b)
        else:
            bins[tid][b][-1][1] = voffs[i + 1]
        m = meta[tid]
        m[0] = voffs[i] if m[0] is None else m[0]
        m[1] = voffs[i + 1]
        m[3 if rec["flag"] & 4 else 2] += 1
        for w in range(beg >> min_shift, ((end - 1) >> min_shift) + 1):
            linear[tid].setdefault(w, voffs[i])
    out = b"CSI\x01" + struct.pack("<iii", min_shift, depth, len(AUX) if foreign else 0) + (AUX if foreign else b"") + struct.pack("<i", n_ref)
    with_records = [t for t in range(n_ref) if meta[t][0] is not None]
    for t in range(n_ref):
        n_win = (max(linear[t]) + 1) if linear[t] else 0
        offs = [linear[t].get(w) for w in range(n_win)]
        if foreign:                                             # from the left: the entry in front, 0 in front of the first
            for w in range(n_win):
                if offs[w] is None:
                    offs[w] = offs[w - 1] if w else 0
        else:                                                   # from the right (a reference's last window always has an entry)
            for w in range(n_win - 2, -1, -1):
                if offs[w] is None:
                    offs[w] = offs[w + 1]
        has = meta[t][0] is not None
        pseudo = has and not (foreign and t == with_records[-1])
        out += struct.pack("<i", len(bins[t]) + (1 if pseudo else 0))
        for k, b in enumerate(sorted(bins[t])):
            chunks = bins[t][b]
            loffset = offs[bin_start_window(b, depth)]
            if foreign:
                merged = [list(chunks[0])]
                for beg, end in chunks[1:]:
                    if beg >> 16 == merged[-1][1] >> 16:
                        merged[-1][1] = end
                    else:
                        merged.append([beg, end])
                chunks = merged
                if k % 3 == 1:
                    loffset = 0
            out += struct.pack("<IQi", b, loffset, len(chunks))
            for beg, end in chunks:
                out += struct.pack("<QQ", beg, end)
        if pseudo:
            out += struct.pack("<IQiQQQQ", first_of(depth + 1) + 1, 0, 2, *meta[t])
    if not foreign:
        out += struct.pack("<Q", n_no_coor)
    return out


def container(data, member=0xFF00, eof=True):
    """``data`` as BGZF members of ``member`` inflated bytes (None: one plain gzip member of everything)."""
    if member is None:
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        return co.compress(data) + co.flush()
    out = b"".join(htslike._bgzf_block(data[at:at + member], 6) for at in range(0, len(data), member))
    return out + (EOF_BLOCK if eof else b"")


def inflate(raw):
    out = b""
    while raw:
        d = zlib.decompressobj(31)
        out += d.decompress(raw)
        assert d.eof
        raw = d.unused_data
    return out


def parse(data):
    assert data[:4] == b"CSI\x01"
    min_shift, depth, l_aux = struct.unpack_from("<iii", data, 4)
    idx = {"min_shift": min_shift, "depth": depth, "aux": data[16:16 + l_aux], "refs": [], "meta": [], "n_no_coor": None}
    p = 16 + l_aux
    n_ref = struct.unpack_from("<i", data, p)[0]
    p += 4
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", data, p)[0]
        p += 4
        ref, meta = {}, None
        for _b in range(n_bin):
            b, loffset, n_chunk = struct.unpack_from("<IQi", data, p)
            p += 16
            chunks = [struct.unpack_from("<QQ", data, p + 16 * c) for c in range(n_chunk)]
            p += 16 * n_chunk
            if b == first_of(depth + 1) + 1:
                meta = (chunks[0][0], chunks[0][1], chunks[1][0], chunks[1][1])
            else:
                assert b < first_of(depth + 1) and b not in ref
                ref[b] = (loffset, chunks)
        idx["refs"].append(ref)
        idx["meta"].append(meta)
    if p < len(data):
        idx["n_no_coor"] = struct.unpack_from("<Q", data, p)[0]
        p += 8
    assert p == len(data)
    return idx


def as_idx(parsed):
    """What svision_amd.io.csi.read_csi returns (its attributes, nothing of its code) in the form :func:`parse` gives."""
    return {"min_shift": parsed.min_shift, "depth": parsed.depth, "aux": parsed.aux, "n_no_coor": parsed.n_no_coor, "meta": list(parsed.meta),
            "refs": [{b: (l, [tuple(c) for c in chunks]) for b, l, chunks in bins} for bins in parsed.bins]}


def regions_match(idx, references, records, voffs, n=500, seed=5):
    """For ``n`` regions (:func:`regions`): the records reached through the index are the records that overlap -> the number checked."""
    for t, beg, end in regions(references, records, n, seed):
        assert reached(idx, records, voffs, t, beg, end) == brute(records, t, beg, end), (t, beg, end)
    return n


def query(idx, tid, beg, end):
    """-> (min_off, chunks): the reader's plan for [beg, end) of reference ``tid``."""
    ref, min_shift, depth = idx["refs"][tid], idx["min_shift"], idx["depth"]
    b = first_of(depth) + (beg >> min_shift)
    min_off = 0
    while True:
        if b in ref:
            min_off = ref[b][0]
            break
        if b == 0:
            break
        b = parent(b)
    chunks = []
    for b in reg2bins(beg, end, min_shift, depth):
        if b in ref:
            chunks += [c for c in ref[b][1] if c[1] > min_off]
    return min_off, sorted(chunks)


def reached(idx, records, voffs, tid, beg, end):
    """The indices of the records a reader gets for the region: it reads every chunk from max(its begin, min_off) to its end and keeps
    what is on ``tid`` and overlaps."""
    min_off, chunks = query(idx, tid, beg, end)
    out = set()
    for c_beg, c_end in chunks:
        for i, rec in enumerate(records):
            if max(c_beg, min_off) <= voffs[i] < c_end and rec["tid"] == tid:
                r_beg, r_end = span_of(rec)
                if r_beg < end and r_end > beg:
                    out.add(i)
    return sorted(out)


def brute(records, tid, beg, end):
    return [i for i, rec in enumerate(records) if rec["tid"] == tid and span_of(rec)[0] < end and span_of(rec)[1] > beg]


# ---- the long-reference list ---------------------------------------------------------------------------------------------------
LONG_REFS = [("long", 700_000_000), ("chrB", 600_000)]
EDGE = 1 << 29


def long_records(seed=7):
    """About 200 sorted records on a 700 Mb reference and a small one: a cluster at 0, one around 2^29 (a record whose last base is
    2^29 - 1, one whose first base is 2^29, one crossing), one at 699,990,000, one record of 2^27 bases, placed unmapped reads and
    a tail without a reference.  No bases: SEQ ``*``."""
    import random
    rng = random.Random(seed)
    recs = []

    def put(tid, pos, span, name, flag=0):
        cigar = [] if flag & 4 else [(span, "M")]
        recs.append(dict(tid=tid, pos=pos, qname=name, flag=flag, mapq=0 if flag & 4 else 60, cigar=cigar, seq="*", tags=[("NM", "i", len(recs) % 7)]))
    for i in range(40):
        put(0, rng.randrange(0, 60_000), rng.randrange(500, 9_000), "zero/%d" % i)
    put(0, 5_000_000, 1 << 27, "huge")
    for i in range(50):
        put(0, EDGE - 40_000 + rng.randrange(0, 80_000), rng.randrange(500, 9_000), "edge/%d" % i)
    put(0, EDGE - 3_000, 3_000, "last_base_below")               # its last base is 2^29 - 1
    put(0, EDGE, 2_500, "first_base_at")
    put(0, EDGE - 1_200, 2_400, "crossing")
    put(0, EDGE + 10, 1, "placed_unmapped", flag=4 | 1 | 64)
    for i in range(40):
        put(0, 699_990_000 + rng.randrange(0, 5_000), rng.randrange(500, 4_000), "far/%d" % i)
    for i in range(50):
        put(1, rng.randrange(0, 590_000), rng.randrange(500, 9_000), "b/%d" % i, flag=(0, 16, 256, 2048)[i % 4])
    put(1, 300_000, 1, "b_unmapped", flag=4)
    recs.sort(key=lambda r: (r["tid"], r["pos"]))               # (stable: equal positions keep their order)
    for i in range(6):
        recs.append(dict(tid=-1, pos=-1, qname="nowhere%d" % i, flag=4, mapq=0, cigar=[], seq="*"))
    return recs


def regions(references, records, n, seed):
    """``n`` (tid, beg, end) for the queries: random ones of every size around the records, and the edges at 0, around 2^29 and at the
    references' ends."""
    import random
    rng = random.Random(seed)
    placed = [r for r in records if r["tid"] >= 0]
    out = []
    for t, (_name, length) in enumerate(references):
        out += [(t, 0, 1), (t, 0, length), (t, length - 1, length), (t, max(length - 20_000, 0), length)]
        if length > EDGE:
            out += [(t, EDGE - 1, EDGE), (t, EDGE, EDGE + 1), (t, EDGE - 1, EDGE + 1), (t, EDGE - 16384, EDGE), (t, EDGE, EDGE + 16384),
                    (t, EDGE - 100_000, EDGE + 100_000), (t, 699_990_000, 699_990_001), (t, 5_000_000 + (1 << 27) - 1, 5_000_000 + (1 << 27) + 1)]
    while len(out) < n:
        rec = rng.choice(placed)
        length = references[rec["tid"]][1]
        beg = min(max(rec["pos"] + rng.randrange(-30_000, 30_000), 0), length - 1)
        end = min(beg + rng.choice([1, 2, 100, 5_000, 16_384, 40_000, 1_000_000, 200_000_000]), length)
        out.append((rec["tid"], beg, max(end, beg + 1)))
    return out


def fake_voffs(records, seed=3):
    """Ascending virtual offsets for a record list that is in no file: n + 1 of them, blocks of a few records each."""
    import random
    rng = random.Random(seed)
    out, coff, off = [], 1000, 0
    for _ in range(len(records) + 1):
        out.append(coff << 16 | off)
        off += rng.randrange(200, 9_000)
        if off >= 0xFF00 or rng.random() < 0.1:
            coff, off = coff + rng.randrange(2_000, 30_000), 0
    return out
