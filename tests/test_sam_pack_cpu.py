"""SAM lines -> the device ingest's packed arrays without a GPU: the phases of svx_sam_pack_count / svx_sam_pack_extract
(svision_amd/csrc/svx_sam_core.hpp) run lane by lane by a stand-alone program (tools/hostwave/sam_pack_main.cpp) under
AddressSanitizer and UBSan -- the text in a heap block of exactly chunk + 64 bytes, every output array in one of exactly its size --
against the host statement of the rules (svision_amd/io/sam.py): status, fields, counts, CIGAR words, name bytes, SEQ bytes."""
import numpy as np
import pytest

from svision_amd.io import sam
from tests import sam_cases, sam_pack_cases as pc, samtext


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return pc.build_program(tmp_path_factory.mktemp("hostwave_pack"))


@pytest.fixture(scope="module")
def case_lines():
    return [samtext.line(rec, sam_cases.REFS) for rec in sam_cases.records()]


def _check(got, lines, with_seq):
    want = pc.wanted_arrays(lines, with_seq)
    assert got["status"].tolist() == want["status"].tolist()
    taken = want["status"] == 0
    assert np.array_equal(got["fields"][:, taken], want["fields"][:, taken]) and np.array_equal(got["counts"], want["counts"])
    assert not got["fields"][:, ~taken].any()
    for k, key in enumerate(("tid", "pos", None, None, "l_seq")):
        if key:
            assert np.array_equal(got[key][taken], want["fields"][k, taken]), key
    assert np.array_equal(got["flag"][taken].view(np.uint16), want["fields"][2, taken]) and np.array_equal(got["mapq"][taken], want["fields"][3, taken])
    # the elements of a line that is not taken are left as they were
    assert (got["tid"][~taken] == np.int32(-0x5A5A5A5B)).all() and (got["mapq"][~taken] == 0xA5).all()
    assert np.array_equal(got["cigar"], want["cigar"]) and got["names"] == want["names"] and got["seq"] == want["seq"]
    return want


@pytest.mark.parametrize("with_seq", [False, True])
def test_every_case_of_the_list(program, tmp_path, case_lines, with_seq):
    want = _check(pc.run_program(program, tmp_path, b"\n".join(case_lines) + b"\n", with_seq), case_lines, with_seq)
    # the 65,536-operation line and the float spellings are the encoder's to refuse, not these kernels'
    assert not want["status"].any() and want["counts"][0].max() == 65536 and (len(want["seq"]) > 70000 // 2) == with_seq


@pytest.mark.parametrize("with_seq", [False, True])
@pytest.mark.parametrize("last_newline", [True, False])
def test_the_shapes(program, tmp_path, with_seq, last_newline):
    host_line, _words = pc.placeholder_line()
    lines = [samtext.line(rec, pc.REFS) for _name, rec in pc.shapes()] + pc.tag_lines()
    lines = lines[:5] + [host_line] + lines[5:]
    got = pc.run_program(program, tmp_path, b"\n".join(lines) + (b"\n" if last_newline else b""), with_seq)
    want = _check(got, lines, with_seq)
    assert want["status"].tolist() == [0] * 5 + [pc.HOST] + [0] * (len(lines) - 6)
    assert want["counts"][0].max() == 70000
    # (the encoders refuse the malformed tags; the floats outside the fast path they leave to the host)
    for line in pc.tag_lines()[:2]:
        with pytest.raises(sam.SamError):
            sam.encode_line(line, pc.TID_OF)


@pytest.mark.parametrize("with_seq", [False, True])
def test_one_line_alone(program, tmp_path, with_seq):
    for name, rec in pc.shapes():
        if name in ("cigar_star", "cigar_65", "cigar_straddle_62", "name_254", "seq_1", "seq_33", "seq_1025", "rname_star_pos_0"):
            for tail in (b"", b"\n"):
                line = samtext.line(rec, pc.REFS)
                _check(pc.run_program(program, tmp_path, line + tail, with_seq), [line], with_seq)
    line, _words = pc.placeholder_line()
    assert pc.run_program(program, tmp_path, line, with_seq)["status"].tolist() == [pc.HOST]


def test_error_codes(program, tmp_path):
    bad = pc.bad_lines()
    assert {code for _line, code in bad} == {sam_cases.E_FIELDS, sam_cases.E_HEADER, sam_cases.E_NAME, sam_cases.E_NUMBER, sam_cases.E_RNAME,
                                             sam_cases.E_CIGAR, sam_cases.E_QUAL}
    lines = [line for line, _code in bad]
    good = samtext.line(sam_cases.records()[3], sam_cases.REFS)
    text = b"\n".join([good] + lines + [good]) + b"\n"
    got = pc.run_program(program, tmp_path, text, True)
    assert got["status"].tolist() == [0] + [code for _line, code in bad] + [0]
    for line, code in bad:                                      # the codes are the host statement's too
        with pytest.raises(sam.SamError) as exc:
            sam.encode_line(line, pc.TID_OF)
        assert exc.value.code == code, line[:60]
    _check(got, [good] + lines + [good], True)
