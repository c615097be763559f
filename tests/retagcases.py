"""Crafted record streams for svx_record_retag_measure / svx_record_retag_write (svision_amd/csrc/svx_recsort_core.hpp: retag_plan,
retag_measure_record, retag_write_record) and their expected rewriting, shared by tests/test_sort_retag_cpu.py (the host program
under sanitizers), tests/test_gpu_record_retag.py (the kernels) and tests/test_gpu_sort_retag.py (the walker, on a merge's records).

Test-side only: ``struct`` and NumPy.  A record is built field by field (:func:`record`); a stream is ``skew`` sentinel bytes and then
the records end to end, the last one ending with the buffer (:func:`place`).  :func:`walk` is the expectation: an independent walk of
one record's optional fields with ``bytes.find`` and slices -> the rewritten record, or None for a malformed one.  A rename table is
``{(tag, old): new}``, the tag a str, the values bytes -- what sort_header.merge_headers hands out per input."""
import struct
import subprocess

import numpy as np

COUNTS = (0, 1, 63, 64, 65, 257)
Z_LENGTHS = (0, 63, 64, 65, 127, 128, 5000)
B_SUBTYPES = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
B_COUNTS = (0, 1, 70000)
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}

# grows by 2, shrinks by 11, and a one-byte value
RENAMES = {("RG", b"grp1"): b"grp1-2", ("PG", b"minimap2.long"): b"mm", ("RG", b"x"): b"x-3"}
ONLY_RG = {("RG", b"grp1"): b"grp1-2"}
WITH_EMPTY = {("RG", b""): b"none-2", ("PG", b"minimap2.long"): b"mm"}


# ---- fields and records ----
def z(tag, value, kind="Z"):
    return tag.encode() + kind.encode() + value + b"\0"


def fixed(tag, kind, seed=0):
    return tag.encode() + kind.encode() + bytes((seed * 37 + 11 * i + 1) % 256 for i in range(FIXED[kind]))


def b_array(tag, sub, count, payload=None):
    if payload is None:
        payload = (np.arange(count * B_SUBTYPES[sub], dtype=np.int64) * 7 + 3).astype(np.uint8).tobytes()
    return tag.encode() + b"B" + sub.encode() + struct.pack("<I", count) + payload


def record(fields=b"", name=b"read\0", n_cigar=1, l_seq=5, seed=0, qual=None):
    """One BAM record: the fixed part, ``name`` (with its NUL), ``n_cigar`` CIGAR words, ``l_seq`` bases and qualities -- seeded
    pseudo-random bytes, ``qual`` given: those -- and ``fields`` behind them; block_size is the length - 4."""
    rng = np.random.default_rng(seed)
    qual = rng.integers(0, 256, l_seq, dtype=np.uint8).tobytes() if qual is None else qual
    assert len(qual) == l_seq and len(name) < 256
    body = (struct.pack("<iiBBHHHIiii", int(rng.integers(-1, 50)), int(rng.integers(-1, 1 << 28)), len(name), int(rng.integers(0, 61)),
                        int(rng.integers(0, 40000)), n_cigar, int(rng.integers(0, 4096)), l_seq, int(rng.integers(-1, 50)),
                        int(rng.integers(-1, 1 << 28)), int(rng.integers(-(1 << 20), 1 << 20)))
            + name + rng.integers(0, 256, 4 * n_cigar, dtype=np.uint8).tobytes() + rng.integers(0, 256, (l_seq + 1) // 2, dtype=np.uint8).tobytes()
            + qual + fields)
    return struct.pack("<i", len(body)) + body


def place(records, skew):
    """-> (bytes uint8, off int64 [n + 1]): ``skew`` sentinel bytes, then the records end to end; the last one ends with the buffer."""
    off = skew + np.concatenate([[0], np.cumsum([len(r) for r in records], dtype=np.int64)]).astype(np.int64)
    return np.frombuffer(b"\xC3" * skew + b"".join(records), np.uint8).copy(), off


# ---- the expectation ----
def walk(rec, renames):
    """One record -> the record with the first RG:Z and the first PG:Z value that ``renames`` holds replaced and block_size set, or None:
    malformed."""
    if len(rec) < 36 or struct.unpack_from("<i", rec, 0)[0] + 4 != len(rec):
        return None
    l_name, n_cigar, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    p = 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    if p > len(rec):
        return None
    out, done = [rec[4:p]], set()
    while p < len(rec):
        if p + 3 > len(rec):
            return None
        tag, kind = rec[p:p + 2].decode("latin-1"), chr(rec[p + 2])
        if kind in FIXED:
            end = p + 3 + FIXED[kind]
        elif kind in "ZH":
            nul = rec.find(b"\0", p + 3)
            if nul < 0:
                return None
            end, value = nul + 1, rec[p + 3:nul]
            if kind == "Z" and tag in ("RG", "PG") and tag not in done and (tag, value) in renames:
                done.add(tag)
                out.append(rec[p:p + 3] + renames[(tag, value)] + b"\0")
                p = end
                continue
        elif kind == "B":
            if p + 8 > len(rec) or chr(rec[p + 3]) not in B_SUBTYPES:
                return None
            end = p + 8 + struct.unpack_from("<I", rec, p + 4)[0] * B_SUBTYPES[chr(rec[p + 3])]
        else:
            return None
        if end > len(rec):
            return None
        out.append(rec[p:end])
        p = end
    body = b"".join(out)
    return struct.pack("<i", len(body)) + body


def z_values(rec, tag):
    """The values of the record's Z fields of ``tag``, in order (a sound record)."""
    l_name, n_cigar, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    p, out = 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq, []
    while p < len(rec):
        kind = chr(rec[p + 2])
        if kind in FIXED:
            end = p + 3 + FIXED[kind]
        elif kind in "ZH":
            end = rec.index(b"\0", p + 3) + 1
            if kind == "Z" and rec[p:p + 2] == tag.encode():
                out.append(rec[p + 3:end - 1])
        else:
            end = p + 8 + struct.unpack_from("<I", rec, p + 4)[0] * B_SUBTYPES[chr(rec[p + 3])]
        p = end
    assert p == len(rec)
    return out


def count_fields(rec):
    """How many optional fields a sound record carries."""
    l_name, n_cigar, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    p, n = 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq, 0
    while p < len(rec):
        kind = chr(rec[p + 2])
        p = p + 3 + FIXED[kind] if kind in FIXED else rec.index(b"\0", p + 3) + 1 if kind in "ZH" else \
            p + 8 + struct.unpack_from("<I", rec, p + 4)[0] * B_SUBTYPES[chr(rec[p + 3])]
        n += 1
    return n


def with_fields(rec, fields):
    """The record with ``fields`` appended behind its own and block_size set."""
    return struct.pack("<i", len(rec) - 4 + len(fields)) + rec[4:] + fields


def expected(data, off, renames):
    """The stream through the two launches -> (the new records end to end uint8, their lengths int64 [n], status)."""
    raw, out, status = data.tobytes(), [], 0
    for r in range(len(off) - 1):
        rec = raw[int(off[r]):int(off[r + 1])]
        new = walk(rec, renames)
        status |= new is None
        out.append(rec if new is None else new)
    return np.frombuffer(b"".join(out), np.uint8).copy(), np.asarray([len(o) for o in out], np.int64), int(status)


def pack(renames):
    """The table as the entry points take it -> (uint8 bytes, int32 offsets [2m + 1])."""
    flat, off = b"", [0]
    for (tag, old), new in renames.items():
        flat += tag.encode() + old
        off.append(len(flat))
        flat += new
        off.append(len(flat))
    return np.frombuffer(flat, np.uint8).copy(), np.asarray(off, np.int32)


def run_host(program, path, data, off, renames):
    """The stand-alone host program on the stream -> (bytes, lengths, status of measure, status of write) as it left them."""
    n = len(off) - 1
    flat, table_off = pack(renames)
    with open(path, "wb") as f:
        f.write(np.asarray([n, len(renames), data.size, flat.size], np.int64).tobytes() + off.astype(np.int64).tobytes() + table_off.tobytes()
                + flat.tobytes() + data.tobytes())
    r = subprocess.run([program, path, path + ".out"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = open(path + ".out", "rb").read()
    status = struct.unpack_from("<ii", raw, 0)
    lens = np.frombuffer(raw, np.int64, n, 8).copy()
    n_out = struct.unpack_from("<q", raw, 8 + 8 * n)[0]
    assert len(raw) == 16 + 8 * n + n_out
    return np.frombuffer(raw, np.uint8, n_out, 16 + 8 * n).copy(), lens, status[0], status[1]


# ---- the streams ----
RG, PG = z("RG", b"grp1"), z("PG", b"minimap2.long")
OTHER = fixed("NM", "i", 1) + z("MD", b"10A5^AC6") + fixed("AS", "s", 2)


def mixed(n, seed=0):
    """n records of every placement of the two tags in turn, with names, CIGARs and sequences of varying length."""
    kinds = (b"", RG, OTHER + RG, RG + OTHER, OTHER + RG + OTHER, RG + PG, PG + OTHER + RG, OTHER + PG, z("RG", b"x") + OTHER,
             z("RG", b"other") + PG, b_array("ML", "C", 300) + RG + z("MM", b"C+m,5,12,0;" * 40), OTHER)
    return [record(kinds[(r + seed) % len(kinds)], name=b"q%d/%d\0" % (seed, r * 7919 % 1000), n_cigar=r % 5, l_seq=(r * 13 + seed) % 41, seed=seed * 1000 + r)
            for r in range(n)]


def placement_cases():
    """Where the tag sits: none, first, last, in the middle, both tags in either order, and tables that hold only one of the two."""
    recs = [record(b"", seed=1), record(b"", name=b"\0", n_cigar=0, l_seq=0, seed=2), record(RG + OTHER, seed=3), record(OTHER + RG, seed=4),
            record(OTHER + RG + OTHER, seed=5), record(RG + PG, seed=6), record(PG + OTHER + RG + OTHER, seed=7), record(RG, seed=8), record(PG, seed=9)]
    return [("placement", recs, RENAMES), ("only RG in the table", recs, ONLY_RG), ("only PG in the table", recs, {("PG", b"minimap2.long"): b"mm"})]


def value_cases():
    """A value that is a strict prefix of an entry, an entry that is a strict prefix of the value, the empty value, a new value that
    is longer (RG) and one that is shorter (PG); the same tag twice: the first that matches counts; RG of another type."""
    recs = [record(z("RG", b"grp") + OTHER, seed=11), record(z("RG", b"grp12") + OTHER, seed=12), record(OTHER + z("RG", b""), seed=13),
            record(z("PG", b"minimap2.lon") + z("RG", b""), seed=14), record(RG + PG, seed=15), record(z("PG", b"minimap2.long.1") + RG, seed=16),
            record(RG + OTHER + RG, seed=17), record(RG + RG, seed=18), record(z("RG", b"nope") + RG + RG, seed=19),
            record(fixed("RG", "i", 5) + OTHER, seed=20), record(fixed("RG", "A", 6) + RG, seed=21), record(z("RG", b"grp1", "H") + PG + PG, seed=22),
            record(b_array("RG", "C", 4, b"grp1") + fixed("PG", "C", 1) + PG, seed=23), record(z("rg", b"grp1") + z("Rg", b"grp1") + z("GR", b"grp1"), seed=24)]
    return [("values", recs, RENAMES), ("values, an empty old value", recs, WITH_EMPTY)]


def type_cases():
    """One field of every type in one record; a B of every subtype with 0, 1 and 70,000 elements (every such record with the largest
    count is longer than 65,535 bytes), the tags behind the arrays."""
    every = b"".join(fixed("X" + k, k, i) for i, k in enumerate(FIXED)) + z("XZ", b"text") + z("XH", b"1AE301", "H") + b_array("XB", "s", 3)
    recs = [record(every + RG + PG, seed=30), record(RG + every + PG, seed=31)]
    for i, sub in enumerate(B_SUBTYPES):
        for count in B_COUNTS:
            recs.append(record(b_array("ML", sub, count) + RG + b_array("fi", sub, count // 3) + PG, l_seq=count % 97, seed=40 + i))
    return [("types", recs, RENAMES)]


def string_cases():
    """Z (and H) values of lengths around the 64-byte steps of the NUL search, at every position of the value's first byte in a step
    of its own, the tag behind them; the value bytes are never 0."""
    recs = []
    for k, length in enumerate(Z_LENGTHS):
        value = bytes(1 + (i * 31 + k) % 255 for i in range(length))
        recs.append(record(z("MM", value) + RG + PG, name=b"n" * (k % 4) + b"\0", seed=60 + k))
        recs.append(record(fixed("NM", "C") + z("XH", value, "H") + PG + z("MD", value) + RG, l_seq=k, seed=70 + k))
        recs.append(record(RG + z("ZZ", value), seed=80 + k))            # (the last field: its NUL is the record's last byte)
    return [("strings", recs, RENAMES)]


def decoy_cases():
    """The bytes ``RGZgrp1\\0`` where no field starts: in another tag's Z value, in a B payload, in the qualities, in the read name."""
    decoy = b"RGZgrp1\0"
    recs = [record(z("CO", b"see RGZgrp1") + fixed("NM", "i"), seed=90), record(z("CO", b"RGZgrp1") + RG, seed=91),
            record(b_array("XB", "C", len(decoy) + 2, b"ab" + decoy) + PG, seed=92), record(b_array("XB", "c", len(decoy), decoy), seed=93),
            record(OTHER, l_seq=len(decoy), qual=decoy, seed=94), record(RG, l_seq=len(decoy) + 3, qual=b"!!!" + decoy, seed=95),
            record(OTHER, name=b"RGZgrp1\0", seed=96), record(PG + RG, name=b"PGZminimap2.long\0", seed=97)]
    return [("decoys", recs, RENAMES)]


def long_case():
    """One record above 65,535 bytes, by its sequence and a long string, between two short ones."""
    return [("long", [record(RG, seed=100), record(z("MM", b"C+m?," + b"1,20,3," * 9000) + PG + b_array("ML", "C", 30000) + RG, l_seq=20001, seed=101),
                      record(PG, seed=102)], RENAMES)]


def malformed(kind):
    """A record that is malformed in the one way ``kind`` names -> its bytes."""
    good = record(OTHER + RG, seed=110)
    cut = lambda fields: record(fields, seed=111)

    def resized(rec, block_size):
        return struct.pack("<i", block_size) + rec[4:]
    return {
        "unknown type": lambda: cut(z("XX", b"v", "Q") + RG),
        "unknown B subtype": lambda: cut(b"XBBZ" + struct.pack("<I", 0) + RG),
        "B subtype A": lambda: cut(b"XBBA" + struct.pack("<I", 1) + b"x" + RG),
        "header cut 1": lambda: cut(RG + b"N"),
        "header cut 2": lambda: cut(RG + b"NM"),
        "fixed value past the end": lambda: cut(RG + b"NMi\1\2\3"),
        "fixed value missing": lambda: cut(RG + b"NMC"),
        "B header cut": lambda: cut(RG + b"XBBC\1\0\0"),
        "B count past the end": lambda: cut(RG + b"XBBs" + struct.pack("<I", 5) + b"\0" * 9),
        "B count huge": lambda: cut(RG + b"XBBI" + struct.pack("<I", 0xFFFFFFFF) + b"\0" * 8),
        "Z without NUL": lambda: cut(RG + b"MDZ" + b"A" * 70),
        "H without NUL": lambda: cut(b"XHH" + b"1F" * 64),
        "block_size too large": lambda: resized(good, len(good) - 4 + 8),
        "block_size too small": lambda: resized(good, len(good) - 4 - 1),
        "block_size negative": lambda: resized(good, -1),
        "shorter than 36": lambda: struct.pack("<i", 16) + b"\7" * 16,
        "four bytes": lambda: struct.pack("<i", 0),
        "fixed part past the end": lambda: resized(good[:20] + struct.pack("<I", 1 << 20) + good[24:], len(good) - 4),
        "l_seq negative": lambda: resized(good[:20] + struct.pack("<i", -5) + good[24:], len(good) - 4),
    }[kind]()


MALFORMED = ("unknown type", "unknown B subtype", "B subtype A", "header cut 1", "header cut 2", "fixed value past the end", "fixed value missing", "B header cut",
             "B count past the end", "B count huge", "Z without NUL", "H without NUL", "block_size too large", "block_size too small",
             "block_size negative", "shorter than 36", "four bytes", "fixed part past the end", "l_seq negative")


def malformed_cases():
    """Every malformed kind between two good records that are rewritten, and as the stream's last record: behind it the buffer ends."""
    before, after = record(RG + PG, seed=120), record(OTHER + RG, seed=121)
    out = []
    for kind in MALFORMED:
        out.append(("malformed: %s" % kind, [before, malformed(kind), after], RENAMES))
        out.append(("malformed at the end: %s" % kind, [before, after, malformed(kind)], RENAMES))
    return out


def shape_cases():
    """Every stream but those of the record counts: (name, records, renames)."""
    return placement_cases() + value_cases() + type_cases() + string_cases() + decoy_cases() + long_case() + malformed_cases()
