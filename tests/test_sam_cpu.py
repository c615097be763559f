"""SAM text -> BAM records without a GPU: the host statement of the rules (svision_amd/io/sam.py) against tests/htslike.py's writer on
every case of tests/sam_cases.py, and the kernels' phases (svision_amd/csrc/svx_sam_core.hpp) run by a stand-alone program
(tools/hostwave/sam_main.cpp) under AddressSanitizer and UBSan -- the text in a heap block of exactly chunk + 64 bytes, the records in
one of exactly their bytes -- against the host statement: line table, lengths, fields, bytes, the refused set and the error codes."""
import gzip
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from svision_amd.io import sam
from tests import htslike, sam_cases, samtext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TID_OF = {name.encode(): i for i, (name, _length) in enumerate(sam_cases.REFS)}


@pytest.fixture(scope="module")
def lines():
    return [samtext.line(rec, sam_cases.REFS) for rec in sam_cases.records()]


@pytest.fixture(scope="module")
def wanted():
    """htslike's record of every case: computed once."""
    return [htslike.encode_record(samtext.for_htslike(rec)) for rec in sam_cases.records()]


def test_the_case_list_holds_what_it_promises():
    names = [name for name, _rec, _refused in sam_cases.cases()]
    assert len(set(names)) == len(names) and len(sam_cases.refused_lines()) == 6
    recs = dict((name, rec) for name, rec, _r in sam_cases.cases())
    assert len(recs["cigar_65536_ops"]["cigar"]) == 65536 and len(recs["cigar_65535_ops"]["cigar"]) == 65535
    assert len(recs["tag_ML_MM"]["tags"][0][2]) > 6000 and len(recs["tag_ML_MM"]["tags"][1][2]) == 5000
    assert len(recs["seq_70000"]["seq"]) == 70000 and len(sam_cases.REFS) == 3366
    # the five levels of reg2bin are all crossed, and every bin level occurs
    levels = set()
    for k, (pos, span) in enumerate(sam_cases.BIN_EDGES):
        b = htslike.reg2bin(pos, pos + span)
        levels.add(sum(b >= first for first in (1, 9, 73, 585, 4681)))
    assert levels == {0, 1, 2, 3, 4, 5}


def test_host_encoder_equals_htslike(lines, wanted):
    for (name, _rec, _refused), line, want in zip(sam_cases.cases(), lines, wanted):
        got = sam.encode_line(line, TID_OF)
        assert got == want, (name, len(got), len(want), next(i for i, (a, b) in enumerate(zip(got + b"\0", want + b"\0")) if a != b))


def test_host_fields_equal_the_records(lines, wanted):
    for line, want, rec in zip(lines, wanted, sam_cases.records()):
        tid, pos, flag, span = sam.fields_of(line, TID_OF)
        assert (tid, pos) == struct.unpack_from("<ii", want, 4) and flag == rec["flag"] and span == htslike.ref_len(rec["cigar"])


def test_header_bytes_equal_htslike(tmp_path):
    text = samtext.header_text(sam_cases.REFS)
    path = str(tmp_path / "h.bam")
    htslike.write_bam(path, sam_cases.REFS, [], header_text=text, index=False)
    want = gzip.decompress(open(path, "rb").read())
    head = sam.parse_header(text.encode())
    assert sam.bam_header_bytes(head) == want
    assert head.references == [r[0] for r in sam_cases.REFS] and head.lengths == [r[1] for r in sam_cases.REFS] and head.sort_order == "unsorted"


def test_read_sam_and_last_line_without_newline(tmp_path, wanted):
    for last_newline in (True, False):
        path = str(tmp_path / ("nl%d.sam" % last_newline))
        with open(path, "wb") as f:
            f.write(sam_cases.case_text(last_newline)[0])
        head, records = sam.read_sam(path)
        assert records == wanted and len(head.references) == sam_cases.N_REFS
    only_header = str(tmp_path / "only.sam")
    with open(only_header, "wb") as f:
        f.write(samtext.header_text(sam_cases.REFS).encode())
    assert sam.read_sam(only_header)[1] == []


@pytest.mark.parametrize("case", sam_cases.errors(), ids=[e[0] for e in sam_cases.errors()])
def test_errors_name_their_line(tmp_path, case):
    name, text, line_no, code = case
    path = str(tmp_path / (name + ".sam"))
    with open(path, "wb") as f:
        f.write(text)
    with pytest.raises(sam.SamError) as exc:
        sam.read_sam(path)
    assert isinstance(exc.value, ValueError)
    if line_no is None:
        assert "@SQ" in str(exc.value)
    else:
        assert "line %d:" % line_no in str(exc.value) and exc.value.code == code, str(exc.value)


def test_a_carriage_return_belongs_to_the_last_field():
    rec = dict(sam_cases.records()[0], tags=[("XZ", "Z", "text")])
    got = sam.encode_line(samtext.line(rec, sam_cases.REFS) + b"\r", TID_OF)
    assert got == htslike.encode_record(dict(rec, tags=[("XZ", "Z", "text\r")]))
    with pytest.raises(sam.SamError):                           # behind QUAL it makes QUAL a byte too long
        sam.encode_line(samtext.line(dict(rec, tags=[], seq="ACGT", qual=bytes(4)), sam_cases.REFS) + b"\r", TID_OF)


def test_is_sam_text():
    assert sam.is_sam_text(b"@HD\tVN:1.6\n") and sam.is_sam_text(samtext.line(sam_cases.records()[0], sam_cases.REFS) + b"\n")
    assert not sam.is_sam_text(b"BAM\x01....") and not sam.is_sam_text(b"\x1f\x8b\x08\x04") and not sam.is_sam_text(b"") \
        and not sam.is_sam_text(b"a\tb\tc\n")


# ---- the chunks of a pass ----
def test_chunks_end_at_line_boundaries(tmp_path):
    body = b"".join(b"r%d\t" % i + b"x" * n + b"\n" for i, n in enumerate((10, 0, 30, 500, 7, 7, 7, 90)))
    head = b"@HD\n@SQ\tSN:a\tLN:5\n"
    for tail in (b"", b"last line without newline"):
        path = str(tmp_path / "c.sam")
        with open(path, "wb") as f:
            f.write(head + body + tail)
        size = len(head + body + tail)
        first_nl = len(head) + body.index(b"\n")
        # a chunk boundary 1 byte before, at and 1 byte behind a newline; chunks smaller than the longest line; one chunk
        for chunk in (first_nl - len(head), first_nl - len(head) + 1, first_nl - len(head) + 2, 1, 5, 64, 100, size, 10 * size):
            places = sam.chunk_places(path, len(head), chunk, block=16)
            assert places[0][0] == len(head) and sum(n for _at, n in places) == size - len(head)
            raw = open(path, "rb").read()
            for k, (at, n) in enumerate(places):
                assert n > 0 and (k == 0 or at == places[k - 1][0] + places[k - 1][1])
                assert raw[at + n - 1:at + n] == b"\n" or at + n == size
                assert n <= chunk or raw[at:at + n - 1].count(b"\n") == 0            # longer than asked: one line only
        assert sam.chunk_places(path, size, 100) == []


# ---- the kernels' phases on the host ----
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_path_factory.mktemp("hostwave") / "sam_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", out, os.path.join(ROOT, "tools", "hostwave", "sam_main.cpp")])
    return out


def _run(program, d, text):
    """The program on ``text`` (alignment lines) -> dict(line_off, len, tid, pos, flag, span, status, out)."""
    paths = [os.path.join(str(d), n) for n in ("text.sam", "names.txt", "out.bin")]
    with open(paths[0], "wb") as f:
        f.write(text)
    with open(paths[1], "wb") as f:
        f.write(b"".join(name.encode() + b"\n" for name, _length in sam_cases.REFS))
    r = subprocess.run([program] + paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = open(paths[2], "rb").read()
    n = struct.unpack_from("<q", raw, 0)[0]
    at = 8
    got = {"line_off": np.frombuffer(raw, "<i8", n + 1, at)}
    at += 8 * (n + 1)
    for key in ("len", "tid", "pos", "flag", "span"):
        got[key] = np.frombuffer(raw, "<i4", n, at)
        at += 4 * n
    got["status"], total = struct.unpack_from("<iq", raw, at)
    got["out"] = raw[at + 12:]
    assert len(got["out"]) == total
    return got


def _extra_lines():
    """Lines that htslike cannot write: every printable byte as a base, a '\\r' at the line's end, signs."""
    base = sam_cases.records()[0]
    every = "".join(chr(c) for c in range(33, 127))
    return [samtext.line(dict(base, qname="every_byte", seq=every, qual=bytes(range(94)), cigar=[(94, "M")]), sam_cases.REFS),
            samtext.line(dict(base, qname="cr", tags=[("XZ", "Z", "text")]), sam_cases.REFS) + b"\r",
            samtext.line(dict(base, qname="plus", tags=[("XF", "f", "+1.25"), ("XG", "f", "1."), ("XH", "f", ".5"), ("XI", "f", "5E+3")]), sam_cases.REFS)]


@pytest.mark.parametrize("last_newline", [True, False])
def test_host_model_equals_the_host_statement(program, tmp_path, lines, last_newline):
    lines = lines + _extra_lines()
    text = b"\n".join(lines) + (b"\n" if last_newline else b"")
    got = _run(program, tmp_path, text)
    starts = np.concatenate([[0], np.cumsum([len(l) + 1 for l in lines])])
    starts[-1] = len(text)
    assert np.array_equal(got["line_off"], starts)
    refused = set(sam_cases.refused_lines())
    assert set(np.flatnonzero(got["len"] == sam.HOST).tolist()) == refused and not (got["len"] < sam.HOST).any()
    at = 0
    for i, line in enumerate(lines):
        want = sam.encode_line(line, TID_OF)
        if i in refused:                                        # (the host encodes the line and patches its fields in)
            continue
        assert (got["tid"][i], got["pos"][i], got["flag"][i], got["span"][i]) == sam.fields_of(line, TID_OF), i
        assert got["len"][i] == len(want), (i, got["len"][i], len(want))
        assert got["out"][at:at + len(want)] == want, i
        at += len(want)
    assert at == len(got["out"]) and got["status"] == 0


def test_host_model_error_codes(program, tmp_path):
    base = sam_cases.records()[0]
    good = samtext.line(dict(base, seq="ACGT", qual=bytes(4), cigar=[(4, "M")], tags=[("XI", "i", 1)]), sam_cases.REFS)

    def edit(col, value):
        cols = good.split(b"\t")
        cols[col] = value
        return b"\t".join(cols)
    bad = [line for _name, text, no, _code in sam_cases.errors() if no is not None for line in [text.split(b"\n")[no - 1]]]
    bad += [edit(0, b""), edit(1, b"65536"), edit(1, b"-1"), edit(1, b""), edit(3, b"2147483648"), edit(4, b"256"), edit(5, b"4"), edit(5, b"M"),
            edit(5, b"4Q"), edit(5, b"1234567890M"), edit(5, b"268435456M"), edit(5, b"2M2"), edit(5, b""), edit(6, b"nowhere"), edit(7, b"x"),
            edit(8, b"2147483648"), edit(9, b"*"), edit(10, b"IIIII"), edit(11, b"XI:i"), edit(11, b"XI-i:1"), edit(11, b"XI:A:ab"),
            edit(11, b"XI:A:"), edit(11, b"XI:i:"), edit(11, b"XI:i:1.5"), edit(11, b"XI:i:-2147483649"), edit(11, b"XI:B:"), edit(11, b"XI:B:c1"),
            edit(11, b"XI:B:q,1"), edit(11, b"XI:B:c,128"), edit(11, b"XI:B:C,-1"), edit(11, b"XI:B:s,1,,2"), edit(11, b"XI:B:S,1,"),
            edit(11, b"XI:B:i,9999999999999"), edit(11, b"XI:Q:1"), good + b"\t", good + b"\tXZ:Z:ok\t"]
    host_decides = [edit(11, b"XI:f:abc"), edit(11, b"XI:f:"), edit(11, b"XI:B:f,1,x"), edit(11, b"XI:f:1e99999")]
    got = _run(program, tmp_path, b"\n".join(bad + host_decides) + b"\n")
    for i, line in enumerate(bad):
        with pytest.raises(sam.SamError) as exc:
            sam.encode_line(line, TID_OF)
        assert got["len"][i] == exc.value.code, (i, line[:80], got["len"][i], exc.value.code)
    # what is no number to the fast path goes to the host, which is the one to refuse it
    assert (got["len"][len(bad):] == sam.HOST).all()
    for line in host_decides[:3]:
        with pytest.raises(sam.SamError):
            sam.encode_line(line, TID_OF)
    assert not got["out"]
