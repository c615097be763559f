"""Crafted record streams for svx_record_tags_measure / svx_record_tags_write (svision_amd/csrc/svx_recsort_core.hpp: tags_new_len,
tags_measure_record, tags_write_record) and their expected filtering, shared by tests/test_sort_tags_cpu.py (the host program under
sanitizers), tests/test_gpu_record_tags.py (the kernels) and tests/test_gpu_sort_tags.py (the walker, as the oracle's filter).

Test-side only: ``struct`` and NumPy; the records are built by tests/retagcases.py's builders (:func:`retagcases.record`, ``place``).
:func:`walk` is the expectation, written from the SAM specification's section 4.2.4 (optional fields) and independent of the C++:
one record -> the record without the removed fields, or None for a malformed one.  A filter is (mode, tags): mode "drop" -- the
fields whose tag is listed go -- or "keep" -- all others go; ``CG`` stays in either mode.  A case is (name, records, drop list);
every case also runs under the complementary keep list (:func:`complement`), which must give the same bytes."""
import struct
import subprocess

import numpy as np

from tests.retagcases import B_SUBTYPES, FIXED, MALFORMED, b_array, fixed, malformed, place, record, z        # noqa: F401  (place: the callers')

COUNTS = (1, 3, 4, 5, 13)                                        # around the four records of a workgroup
Z_LENGTHS = (0, 62, 63, 64, 65, 127, 128, 129)                   # around the 64-byte steps of the NUL search
TABLE_BYTES = 8192
DROP = ("XD", "YD", "fi")                                        # the drop list of most cases: fields with these tags go


# ---- the expectation ----
def removes(tag, mode, tags):
    """Whether a field of ``tag`` (two latin-1 characters) goes under the filter."""
    if tag == "CG":
        return False
    return tag in tags if mode == "drop" else tag not in tags


def field_ends(rec):
    """The optional fields of one record as the specification lays them out -> (p, [(start, end, tag)]): p the offset of the first,
    the fields in order; None: the record is malformed -- shorter than its fixed part says, block_size + 4 not its length, a field
    header cut by the end, a type that is none of A c C s S i I f Z H B, a B subtype that is none of c C s S i I f, a value or an array
    past the end, a Z / H without NUL."""
    if len(rec) < 36 or struct.unpack_from("<i", rec, 0)[0] + 4 != len(rec):
        return None
    l_read_name, n_cigar_op, l_seq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    p = first = 36 + l_read_name + 4 * n_cigar_op + (l_seq + 1) // 2 + l_seq
    if p > len(rec):
        return None
    out = []
    while p < len(rec):
        if len(rec) - p < 3:
            return None
        tag, kind = rec[p:p + 2].decode("latin-1"), rec[p + 2:p + 3]
        if kind in (b"A", b"c", b"C"):
            end = p + 4
        elif kind in (b"s", b"S"):
            end = p + 5
        elif kind in (b"i", b"I", b"f"):
            end = p + 7
        elif kind in (b"Z", b"H"):
            nul = rec.find(b"\0", p + 3)
            if nul < 0:
                return None
            end = nul + 1
        elif kind == b"B":
            if len(rec) - p < 8:
                return None
            width = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}.get(rec[p + 3:p + 4])
            if width is None:
                return None
            end = p + 8 + width * struct.unpack_from("<I", rec, p + 4)[0]
        else:
            return None
        if end > len(rec):
            return None
        out.append((p, end, tag))
        p = end
    return first, out


def walk(rec, mode, tags):
    """One record -> the record without the fields the filter removes, block_size set, or None: malformed."""
    got = field_ends(rec)
    if got is None:
        return None
    first, fields = got
    body = rec[4:first] + b"".join(rec[a:b] for a, b, tag in fields if not removes(tag, mode, tags))
    return struct.pack("<i", len(body)) + body


def tags_seen(records):
    """Every tag that a field of the sound records carries (a malformed record stays as it is under any filter) -- for :func:`complement`."""
    seen = []
    for rec in records:
        got = field_ends(rec)
        for _a, _b, tag in (got[1] if got else []):
            if tag not in seen:
                seen.append(tag)
    return seen


def complement(records, drop):
    """The keep list that removes from ``records`` what the drop list ``drop`` removes: every tag they carry that is not in it."""
    return tuple(t for t in tags_seen(records) if t not in drop and t != "CG")


def expected(data, off, mode, tags):
    """The stream through the two launches -> (the new records end to end uint8, their lengths int64 [n], status)."""
    raw, out, status = data.tobytes(), [], 0
    for r in range(len(off) - 1):
        rec = raw[int(off[r]):int(off[r + 1])]
        new = walk(rec, mode, tags)
        status |= new is None
        out.append(rec if new is None else new)
    return np.frombuffer(b"".join(out), np.uint8).copy(), np.asarray([len(o) for o in out], np.int64), int(status)


def bitmap(mode, tags):
    """The table as the entry points take it, built here bit by bit -> int32 [2048]: bit (t0 | t1 << 8) set = removed."""
    bits = np.full(1 << 16, mode == "keep", bool)
    for tag in tuple(tags) + (("CG",) if mode == "keep" else ()):
        raw = tag.encode("latin-1")
        bits[raw[0] | raw[1] << 8] = mode == "drop"
    bits[ord("C") | ord("G") << 8] = False
    return np.packbits(bits, bitorder="little").view("<i4")


def run_host(program, path, data, off, mode, tags):
    """The stand-alone host program on the stream -> (bytes, lengths, status of measure, status of write) as it left them."""
    n = len(off) - 1
    with open(path, "wb") as f:
        f.write(np.asarray([n, data.size], np.int64).tobytes() + off.astype(np.int64).tobytes() + bitmap(mode, tags).tobytes() + data.tobytes())
    r = subprocess.run([program, path, path + ".out"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = open(path + ".out", "rb").read()
    status = struct.unpack_from("<ii", raw, 0)
    lens = np.frombuffer(raw, np.int64, n, 8).copy()
    n_out = struct.unpack_from("<q", raw, 8 + 8 * n)[0]
    assert len(raw) == 16 + 8 * n + n_out
    return np.frombuffer(raw, np.uint8, n_out, 16 + 8 * n).copy(), lens, status[0], status[1]


# ---- the streams ----
K1, K2, K3 = fixed("NM", "i", 1), z("MD", b"10A5^AC6"), fixed("AS", "s", 2)          # kept
R1, R2 = fixed("XD", "i", 3), z("YD", b"gone with the filter")                      # removed under DROP


def of_type(tag, kind, seed=0):
    """One field of ``tag`` whose type is ``kind``: A c C s S i I f, Z, H, or B + a subtype ("Bc" ... "Bf")."""
    if kind in FIXED:
        return fixed(tag, kind, seed)
    if kind in "ZH":
        return z(tag, b"1AE301", kind)
    return b_array(tag, kind[1], 3 + seed % 5)


TYPES = tuple(FIXED) + ("Z", "H") + tuple("B" + sub for sub in B_SUBTYPES)


def mixed(n, seed=0):
    """n records of every placement in turn, with names, CIGARs and sequences of varying length."""
    kinds = (b"", R1, K1 + R1, R1 + K1, K1 + R2 + K2, R1 + R2, K1 + R1 + K2 + R2 + K3, R2 + K1 + R1, K1 + K2 + K3,
             b_array("fi", "C", 300) + K1 + z("MM", b"C+m,5,12,0;" * 40), R1 + R1, K3 + b_array("fi", "S", 77) + b_array("ML", "C", 90) + R2)
    return [record(kinds[(r + seed) % len(kinds)], name=b"q%d/%d\0" % (seed, r * 7919 % 1000), n_cigar=r % 5, l_seq=(r * 13 + seed) % 41, seed=seed * 1000 + r)
            for r in range(n)]


def placement_cases():
    """No optional field; the one field removed; the first, a middle and the last field removed; all removed; two adjacent removed;
    removed and kept fields alternating, so that runs of one kept field occur; the same tag twice, both removed."""
    recs = [record(b"", seed=1), record(b"", name=b"\0", n_cigar=0, l_seq=0, seed=2), record(R1, seed=3), record(R2, name=b"\0", n_cigar=0, l_seq=0, seed=4),
            record(R1 + K1 + K2, seed=5), record(K1 + R2 + K2, seed=6), record(K1 + K2 + R1, seed=7), record(R1 + R2 + R1, seed=8),
            record(K1 + R1 + R2 + K2, seed=9), record(R1 + K1 + R2 + K2 + R1 + K3 + R2, seed=10), record(K1 + R1 + K2 + R2 + K3, seed=11),
            record(R1 + K1 + fixed("XD", "C", 9), seed=12), record(z("YD", b"one") + z("YD", b"two, another length"), seed=13),
            record(K1 + K2 + K3, seed=14)]
    return [("placement", recs, DROP), ("placement, an empty drop set for these records", recs, ("ZZ",)), ("placement, everything listed", recs, ("XD", "YD", "NM", "MD", "AS"))]


def type_cases():
    """Every type A c C s S i I f Z H and B with every subtype, once as the removed field between two kept ones and once as a kept
    field that is stepped over between two removed ones; and one record that carries them all, alternating."""
    recs = []
    for i, kind in enumerate(TYPES):
        recs.append(record(K1 + of_type("XD", kind, i) + K3, seed=20 + i))
        recs.append(record(R1 + of_type("T%d" % (i % 10), kind, i) + R2, l_seq=i, seed=40 + i))
    recs.append(record(b"".join(of_type("XD" if i % 2 else "K%d" % (i % 10), kind, i) for i, kind in enumerate(TYPES)), seed=60))
    return [("types", recs, DROP)]


def string_cases():
    """Z (and H) values of lengths around the 64-byte steps of the NUL search, removed and kept, behind names of every length mod 4;
    as the record's last bytes; the value bytes are never 0."""
    recs = []
    for k, length in enumerate(Z_LENGTHS):
        value = bytes(1 + (i * 31 + k) % 255 for i in range(length))
        recs.append(record(K1 + z("YD", value) + K3, name=b"n" * (k % 4) + b"\0", seed=70 + k))
        recs.append(record(R1 + z("MM", value) + R2 + z("XH", value[:length // 2 * 2], "H") + R1, l_seq=k, seed=80 + k))
        recs.append(record(K1 + z("YD", value), seed=90 + k))           # (removed, and the record's last byte run)
        recs.append(record(R1 + z("ZZ", value), seed=100 + k))          # (kept: its NUL is the record's last byte)
    return [("strings", recs, DROP)]


def decoy_cases():
    """Bytes that spell a listed tag with a type and a count where no field starts: in a kept Z value, in a kept B array's data, in
    the qualities and in the read name; and in a REMOVED field's value, behind which the chain must go on at the right byte."""
    decoy = b"XDBC" + struct.pack("<I", 40) + b"YDZ"
    text = b"XDBC(YDZxx"                                             # (no NUL inside: a Z value)
    recs = [record(z("CO", text) + R1 + K1, seed=110), record(K1 + z("CO", b"see XDi1234 and YDZ") + R2, seed=111),
            record(b_array("XB", "C", len(decoy) + 2, b"ab" + decoy) + R1 + K3, seed=112), record(b_array("XB", "c", len(decoy), decoy), seed=113),
            record(K1 + R1, l_seq=len(decoy), qual=decoy, seed=114), record(R2 + K2, name=b"XDZname\0", seed=115),
            record(b_array("XD", "C", len(decoy), decoy) + K1 + z("YD", b"NMi1234") + K2, seed=116)]
    return [("decoys", recs, DROP)]


def array_cases():
    """B arrays of no element, removed and kept; one B:S array of 20,000 elements -- a kinetics-sized field -- removed from between two
    kept fields, and kept between two removed ones: the record is longer than 65,535 bytes."""
    recs = [record(K1 + b_array("XD", "S", 0) + K2, seed=120), record(R1 + b_array("ML", "f", 0) + R2, seed=121), record(b_array("fi", "C", 0), seed=122),
            record(K1 + b_array("fi", "S", 20000) + K2, l_seq=300, seed=123), record(R1 + b_array("ip", "S", 20000) + R2, seed=124),
            record(b_array("fi", "C", 5000) + b_array("fp", "C", 5000) + K1 + b_array("XD", "C", 5000) + z("MM", b"C+m?," + b"1,20,3," * 700) + b_array("ML", "C", 2100), l_seq=5000, seed=125)]
    return [("arrays", recs, DROP), ("arrays, the kinetics dropped", recs, ("fi", "fp", "ri", "rp"))]


def cg_record(seed=130, more=b""):
    """A record with the placeholder CIGAR (<l_seq>S<ref span>N) and its real CIGAR in CG:B:I."""
    return record(K1 + b_array("CG", "I", 70000 // 4) + more, n_cigar=2, l_seq=11, seed=seed)


def cg_cases():
    """``CG`` is implied in every keep list -- the empty one included -- and stays; a CG of another type stays too."""
    recs = [cg_record(), cg_record(131, R1 + K2), record(fixed("CG", "i", 4) + R1, seed=132), record(K1 + R2, seed=133)]
    return [("CG under a keep list without it", recs, ("XD", "YD", "MD")), ("CG under an empty keep list", recs, ("XD", "YD", "MD", "NM"))]


def malformed_cases():
    """Every malformed kind of retagcases between two good records that are filtered, and as the stream's last record: behind it the
    buffer ends.  Its tags are listed, so a record that was taken apart in spite of its fault would show."""
    before, after = record(K1 + R1 + K2, seed=140), record(R2 + z("RG", b"grp1") + K1, seed=141)
    out = []
    for kind in MALFORMED:
        out.append(("malformed: %s" % kind, [before, malformed(kind), after], DROP + ("RG", "XX", "XB", "XH")))
        out.append(("malformed at the end: %s" % kind, [before, after, malformed(kind)], DROP + ("RG", "XX", "XB", "XH")))
    return out


def shape_cases():
    """Every stream but those of the record counts: (name, records, drop list)."""
    return placement_cases() + type_cases() + string_cases() + decoy_cases() + array_cases() + cg_cases() + malformed_cases()


def filters(records, drop):
    """The two filters a case runs under: its drop list, and the keep list that removes the same fields."""
    return (("drop", tuple(drop)), ("keep", complement(records, drop)))
