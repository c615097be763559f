"""The lines of the SAM pack tests (tests/test_sam_pack_cpu.py, tests/test_gpu_sam_pack.py) beyond tests/sam_cases.py, what
svision_amd/io/sam.py says of a line -- the yardstick of svx_sam_pack_count / svx_sam_pack_extract --, and the reader of what
tools/hostwave/sam_pack_main.cpp writes."""
import os
import struct
import subprocess

import numpy as np

from svision_amd.io import sam
from tests import sam_cases, samtext

REFS = sam_cases.REFS
TID_OF = {name.encode(): i for i, (name, _length) in enumerate(REFS)}
SEQ_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025)
IUPAC = "=ACMGRSVTWYHKDBNacmgrsvtwyhkdbn"
HOST = -1


def _rec(name, **kw):
    return sam_cases._rec(name, **kw)


def many_ops(n=70000):
    return [(1 + i % 7, "MID"[i % 3]) for i in range(n)]


def shapes():
    """[(name, record)]: the shapes of the issue's list, every one a line both kernels take (status 0)."""
    out = [("cigar_star", _rec("cigar_star")), ("cigar_1", _rec("cigar_1", cigar=[(1, "M")]))]
    for n in (63, 64, 65):
        out.append(("cigar_%d" % n, _rec("cigar_%d" % n, tid=2, cigar=[(1 + i % 29, "MIDNSHP=X"[i % 9]) for i in range(n)])))
    out.append(("cigar_70000", _rec("cigar_70000", tid=3, pos=77, cigar=many_ops())))
    # an operation's digits across the 64-byte steps of the field: the number begins 1 .. 7 bytes in front of byte 64 and of byte 128
    for lead in range(57, 64):
        front = [(1, "M")] * (lead // 2) + ([(7, "I")] if lead % 2 == 0 else [(12, "I")])       # `lead` or lead + 1 bytes
        out.append(("cigar_straddle_%d" % lead, _rec("straddle_%d" % lead, cigar=front + [(1234567, "D")] + [(3, "M")] * 28 + [(123456789, "N"), (2, "M")])))
    out.append(("name_1", _rec("n")))
    out.append(("name_254", _rec("N" * 254, cigar=[(3, "M")])))
    for k, n in enumerate(SEQ_LENGTHS):
        seq = "".join(IUPAC[(i * 7 + k) % len(IUPAC)] for i in range(n))
        out.append(("seq_%d" % n, _rec("seq_%d" % n, pos=10 + n, cigar=[(n, "M")], seq=seq, qual=bytes(i % 94 for i in range(n)) if k % 2 else None)))
    out.append(("seq_star", _rec("seq_star", cigar=[(4, "M")])))
    out.append(("rname_star_pos_0", _rec("unplaced", tid=-1, pos=-1, flag=4, seq="ACGTN", qual=bytes(5))))
    # two operations that are no placeholder: another length than l_seq, another letter
    out.append(("two_ops_other_length", _rec("two_a", cigar=[(4, "S"), (9, "N")], seq="ACGTA")))
    out.append(("two_ops_other_letter", _rec("two_b", cigar=[(5, "S"), (9, "M")], seq="ACGTA")))
    return out


def tag_lines():
    """Lines whose tags the encoders refuse or hand to the host, and which the pack kernels take: the tags are not read."""
    base = _rec("tagged", cigar=[(4, "M")], seq="ACGT", qual=bytes(4))
    good = samtext.line(base, REFS)
    return [good + b"\tXI:Q:1", good + b"\tXI:i:", good + b"\tXF:f:1e30", good + b"\tXG:B:f,1,nan", good + b"\t", good + b"\tXI:i:4294967296"]


def placeholder_line(n_real=70, l_seq=10):
    """``<l_seq>S<n>N`` beside a CG:B:I tag, as `minimap2 -L` writes it -> (the line, the real CIGAR words)."""
    real = [(1 + i % 5, "MID"[i % 3]) for i in range(n_real)]
    words = [n << 4 | "MIDNSHP=X".index(op) for n, op in real]
    span = sum(n for n, op in real if op in "MDN=X")
    rec = _rec("long_cigar", tid=1, pos=4242, cigar=[(l_seq, "S"), (span, "N")], seq="ACGTACGTAC"[:l_seq], qual=bytes(l_seq),
               tags=[("NM", "i", 5), ("CG", "BI", words), ("XZ", "Z", "behind")])
    return samtext.line(rec, REFS), words


def bad_lines():
    """[(line, the code)]: one fault each in the first eleven fields, every code they can have, QUAL of another length among them."""
    good = samtext.line(_rec("good", pos=100, cigar=[(4, "M")], seq="ACGT", qual=bytes(4)), REFS)

    def edit(col, value):
        cols = good.split(b"\t")
        cols[col] = value
        return b"\t".join(cols)
    E = sam_cases
    return [(b"", E.E_FIELDS), (b"\t".join(good.split(b"\t")[:10]), E.E_FIELDS), (b"@CO\tlate", E.E_HEADER),
            (edit(0, b""), E.E_NAME), (edit(0, b"n" * 255), E.E_NAME),
            (edit(1, b"65536"), E.E_NUMBER), (edit(1, b"-1"), E.E_NUMBER), (edit(1, b""), E.E_NUMBER), (edit(3, b"12x"), E.E_NUMBER),
            (edit(3, b"2147483648"), E.E_NUMBER), (edit(4, b"256"), E.E_NUMBER), (edit(7, b"x"), E.E_NUMBER), (edit(8, b"2147483648"), E.E_NUMBER),
            (edit(2, b"chrUnknown"), E.E_RNAME), (edit(6, b"nowhere"), E.E_RNAME),
            (edit(5, b"4"), E.E_CIGAR), (edit(5, b"M"), E.E_CIGAR), (edit(5, b"4Q"), E.E_CIGAR), (edit(5, b"1234567890M"), E.E_CIGAR),
            (edit(5, b"268435456M"), E.E_CIGAR), (edit(5, b"2M2"), E.E_CIGAR), (edit(5, b""), E.E_CIGAR),
            (edit(10, b"III"), E.E_QUAL), (edit(10, b"IIIII"), E.E_QUAL), (edit(9, b"*"), E.E_QUAL)]


def expected(line, with_seq, tid_of=TID_OF):
    """What io/sam.py says of the line's first eleven fields -> (status, (tid, pos, flag, mapq, l_seq), the CIGAR words, the name bytes,
    the SEQ bytes); an error: (its code, None, ...)."""
    core = b"\t".join(line.split(b"\t")[:11])
    try:
        rec = sam.encode_line(core, tid_of)
        tid, pos, flag, _span = sam.fields_of(core, tid_of)
    except sam.SamError as exc:
        return exc.code, None, None, None, None
    f = core.split(b"\t")
    words = [] if f[5] == b"*" else sam.cigar_words(f[5])[0]
    _tid, _pos, l_name, mapq, _bin, n_cig, _flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
    if len(words) == 2 and words[0] == (l_seq << 4 | 4) and words[1] & 15 == 3:
        return HOST, None, None, None, None
    seq_at = 36 + l_name + 4 * n_cig                             # (beyond 65,535 operations the record holds the two placeholder words)
    return 0, (tid, pos, flag, mapq, l_seq), words, f[0] + b"\n", rec[seq_at:seq_at + (l_seq + 1) // 2] if with_seq else b""


def wanted_arrays(lines, with_seq, tid_of=TID_OF):
    """The lines' packed arrays by :func:`expected`, the lines that are not taken left out of the three data arrays -> dict(status,
    fields [5, n], counts [3, n], cigar, names, seq)."""
    status, fields, counts = np.zeros(len(lines), np.int32), np.zeros((5, len(lines)), np.int32), np.zeros((3, len(lines)), np.int32)
    cigar, names, seq = [], [], []
    for i, line in enumerate(lines):
        st, fl, words, name, bases = expected(line, with_seq, tid_of)
        status[i] = st
        if st == 0:
            fields[:, i] = fl
            counts[:, i] = len(words), len(name), len(bases)
            cigar += words
            names.append(name)
            seq.append(bases)
    return dict(status=status, fields=fields, counts=counts, cigar=np.array(cigar, np.uint32), names=b"".join(names), seq=b"".join(seq))


def build_program(directory):
    import shutil
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(str(directory), "sam_pack_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", out, os.path.join(root, "tools", "hostwave", "sam_pack_main.cpp")])
    return out


def run_program(program, directory, text, with_seq, refs=REFS):
    """The host program on ``text`` -> dict(status, fields, counts, tid, pos, l_seq, flag, mapq, cigar, names, seq)."""
    paths = [os.path.join(str(directory), n) for n in ("text.sam", "names.txt", "out.bin")]
    with open(paths[0], "wb") as f:
        f.write(text)
    with open(paths[1], "wb") as f:
        f.write(b"".join(name.encode() + b"\n" for name, _length in refs))
    r = subprocess.run([program] + paths + [str(int(with_seq))], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = open(paths[2], "rb").read()
    n = struct.unpack_from("<q", raw, 0)[0]
    at, got = 8, {}
    for key, dtype, count in (("status", "<i4", n), ("fields", "<i4", 5 * n), ("counts", "<i4", 3 * n), ("tid", "<i4", n), ("pos", "<i4", n),
                              ("l_seq", "<i4", n), ("flag", "<i2", n), ("mapq", "u1", n)):
        got[key] = np.frombuffer(raw, dtype, count, at)
        at += count * np.dtype(dtype).itemsize
    got["fields"], got["counts"] = got["fields"].reshape(5, n), got["counts"].reshape(3, n)
    totals = struct.unpack_from("<3q", raw, at)
    at += 24
    got["cigar"] = np.frombuffer(raw, "<u4", totals[0], at)
    at += 4 * totals[0]
    got["names"], got["seq"] = raw[at:at + totals[1]], raw[at + totals[1]:at + totals[1] + totals[2]]
    assert at + totals[1] + totals[2] == len(raw)
    return got
