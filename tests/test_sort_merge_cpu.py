"""Several inputs merged into one sorted BAM (svision_amd/sort.py), the parts that need no GPU: the header merge (merge_headers) on
crafted header texts -- every expectation is a text, a list or a dict lookup written here -- and the routine of svx_record_retid
(svision_amd/csrc/svx_recsort_core.hpp) in a stand-alone program (tools/hostwave/retid_main.cpp) under AddressSanitizer and UBSan,
the record bytes in a heap block of exactly their size, against tests/retidcases.py's struct.pack_into translation."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from svision_amd import sort
from tests import retidcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = [("chr1", 1000), ("chr2", 2000), ("chr3", 3000), ("chrM", 16)]


def _sq(refs):
    return "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)


def _part(name, text, refs):
    return (name, text, [r[0] for r in refs], [r[1] for r in refs])


def _lookup(own, merged):
    at = {name: i for i, (name, _n) in enumerate(merged)}
    return [at[name] for name, _n in own]


def test_identical_dictionaries_give_identity_tables():
    text = "@HD\tVN:1.6\tSO:unsorted\n" + _sq(REFS) + "@PG\tID:aln\tPN:aln\n"
    m = sort.merge_headers([_part("a.bam", text, REFS), _part("b.bam", text, REFS), _part("c.sam", text, REFS)])
    assert m.references == [r[0] for r in REFS] and m.lengths == [r[1] for r in REFS]
    assert len(m.maps) == 3 and all(t.dtype == np.int32 and t.tolist() == [0, 1, 2, 3] for t in m.maps)
    assert m.text == "@HD\tVN:1.6\tSO:coordinate\n" + _sq(REFS) + "@PG\tID:aln\tPN:aln\n"


def test_permuted_extended_and_subset_dictionaries():
    a = REFS[:3]
    b = [REFS[2], REFS[0], REFS[1]]                             # permuted
    c = [REFS[1], ("extra", 77), REFS[3]]                       # extended: two references no earlier input has
    d = [REFS[3], REFS[0]]                                      # a subset of what is there by now
    parts = [_part(n, "@HD\tVN:1.6\n" + _sq(r), r) for n, r in (("a", a), ("b", b), ("c", c), ("d", d))]
    m = sort.merge_headers(parts)
    merged = a + [("extra", 77), REFS[3]]                       # first appearance, the inputs in list order
    assert list(zip(m.references, m.lengths)) == merged
    for table, own in zip(m.maps, (a, b, c, d)):
        assert table.dtype == np.int32 and table.tolist() == _lookup(own, merged)
    assert m.maps[0].tolist() == [0, 1, 2] and m.maps[1].tolist() == [2, 0, 1]
    assert m.text == "@HD\tVN:1.6\tSO:coordinate\n" + _sq(merged)


def test_the_first_occurrence_of_an_sq_line_is_kept_whole():
    a = "@SQ\tSN:chr1\tLN:1000\tM5:aaaa\tUR:file:/a.fa\n"
    b = "@SQ\tSN:chr2\tLN:2000\tAS:b\n@SQ\tSN:chr1\tLN:1000\tM5:other\n"
    m = sort.merge_headers([_part("a", a, REFS[:1]), _part("b", b, [REFS[1], REFS[0]])])
    assert m.text == "@HD\tVN:1.6\tSO:coordinate\n" + a + "@SQ\tSN:chr2\tLN:2000\tAS:b\n"
    assert m.maps[1].tolist() == [1, 0]


def test_conflicts_name_both_files():
    a = _part("/data/cell1.bam", _sq(REFS[:2]) + "@RG\tID:rg\tSM:one\n", REFS[:2])
    other_length = [REFS[0], ("chr2", 2001)]
    with pytest.raises(sort.SortWriteError) as exc:
        sort.merge_headers([a, _part("/data/cell2.bam", _sq(other_length), other_length)])
    msg = str(exc.value)
    assert "/data/cell1.bam" in msg and "/data/cell2.bam" in msg and "chr2" in msg and "2000" in msg and "2001" in msg
    with pytest.raises(sort.SortWriteError) as exc:
        sort.merge_headers([a, _part("/data/cell3.sam", _sq(REFS[:2]) + "@RG\tID:rg\tSM:two\n", REFS[:2])])
    msg = str(exc.value)
    assert "/data/cell1.bam" in msg and "/data/cell3.sam" in msg and "rg" in msg and "RG:Z" in msg
    # the same @RG line in both: once
    m = sort.merge_headers([a, _part("b", _sq(REFS[:2]) + "@RG\tID:rg\tSM:one\n@RG\tID:rg2\tSM:one\n", REFS[:2])])
    assert m.text.count("@RG\t") == 2 and m.text.index("ID:rg\t") < m.text.index("ID:rg2\t")


def test_pg_rename_with_a_pp_chain():
    sq = _sq(REFS[:1])
    a = sq + "@PG\tID:minimap2\tPN:minimap2\tCL:minimap2 -a ref.fa one.fq\n@PG\tID:samtools\tPN:samtools\tPP:minimap2\tCL:samtools view -b\n"
    b = sq + "@PG\tID:minimap2\tPN:minimap2\tCL:minimap2 -a ref.fa two.fq\n@PG\tID:samtools\tPN:samtools\tPP:minimap2\tCL:samtools view -b\n" \
        "@PG\tID:other\tPN:other\n"
    c = sq + "@PG\tID:minimap2\tPN:minimap2\tCL:minimap2 -a ref.fa one.fq\n@PG\tID:other\tPN:other\n"
    m = sort.merge_headers([_part("a", a, REFS[:1]), _part("b", b, REFS[:1]), _part("c", c, REFS[:1])])
    assert m.text == ("@HD\tVN:1.6\tSO:coordinate\n" + sq
                      + "@PG\tID:minimap2\tPN:minimap2\tCL:minimap2 -a ref.fa one.fq\n"
                      + "@PG\tID:samtools\tPN:samtools\tPP:minimap2\tCL:samtools view -b\n"
                      + "@PG\tID:minimap2-2\tPN:minimap2\tCL:minimap2 -a ref.fa two.fq\n"
                      # (its PP follows the rename, which makes the line another one than the first input's: renamed too)
                      + "@PG\tID:samtools-2\tPN:samtools\tPP:minimap2-2\tCL:samtools view -b\n"
                      + "@PG\tID:other\tPN:other\n")


def test_other_lines_once_and_in_input_order():
    sq = _sq(REFS[:1])
    a = "@HD\tVN:1.5\tSO:queryname\tGO:query\n" + sq + "@CO\tfirst\n@CO\tshared\n"
    b = "@HD\tVN:1.4\tSO:unsorted\n" + sq + "@CO\tshared\n@CO\tsecond\n@XY\tzz:1\n"
    m = sort.merge_headers([_part("a", a, REFS[:1]), _part("b", b, REFS[:1])])
    assert m.text == "@HD\tVN:1.5\tSO:coordinate\n" + sq + "@CO\tfirst\n@CO\tshared\n@CO\tsecond\n@XY\tzz:1\n"


def test_a_first_input_without_hd_and_a_headerless_part():
    sq = _sq(REFS[:2])
    m = sort.merge_headers([_part("a", sq, REFS[:2]), _part("b", "@HD\tVN:1.0\tSO:unsorted\n" + sq, REFS[:2]), _part("bare.sam", "", [])])
    assert m.text == "@HD\tVN:1.6\tSO:coordinate\n" + sq
    assert [t.tolist() for t in m.maps] == [[0, 1], [0, 1], []]
    # a headerless part first: the dictionary is the second input's
    m = sort.merge_headers([_part("bare.sam", "", []), _part("b", "@HD\tVN:1.0\n" + sq + "@CO\tx\n", REFS[:2])])
    assert m.references == ["chr1", "chr2"] and m.text == "@HD\tVN:1.6\tSO:coordinate\n" + sq + "@CO\tx\n"
    with pytest.raises(sort.SortWriteError, match="@SQ"):
        sort.merge_headers([_part("bare.sam", "", []), _part("bare2.sam", "", [])])


def test_one_input_is_sorted_header_text():
    for text in ("@HD\tVN:1.3\tSO:unsorted\tGO:none\tXX:1\n" + _sq(REFS) + "@CO\tx\n@CO\tx\n", _sq(REFS), _sq(REFS).rstrip("\n"), "@CO\tonly\n" + _sq(REFS)):
        m = sort.merge_headers([_part("a", text, REFS)])
        assert m.text == sort.sorted_header_text(text) and m.maps[0].tolist() == [0, 1, 2, 3] and m.references == [r[0] for r in REFS]


def test_a_dictionary_entry_without_a_text_line_gets_one():
    """A BAM carries its dictionary in binary; a text that lacks the @SQ line of a reference another input brings gets the plain one."""
    m = sort.merge_headers([_part("a", "@HD\tVN:1.6\n" + _sq(REFS[:1]), REFS[:1]), _part("b", "@CO\tno sq lines\n", REFS[:2])])
    assert m.text == "@HD\tVN:1.6\tSO:coordinate\n" + _sq(REFS[:2]) + "@CO\tno sq lines\n" and m.maps[1].tolist() == [0, 1]


def test_input_paths():
    assert sort.input_paths("a.bam") == ["a.bam"] and sort.input_paths(["a.bam"]) == ["a.bam"] and sort.input_paths(("a", "b")) == ["a", "b"]
    with pytest.raises(ValueError):
        sort.input_paths([])
    with pytest.raises(ValueError):
        sort.sort_bam([], "never.bam")
    assert "retid" in sort.STAGES


# ---- the routine of svx_record_retid on the host ----
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_path_factory.mktemp("hostwave") / "retid_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", out, os.path.join(ROOT, "tools", "hostwave", "retid_main.cpp")])
    return out


@pytest.mark.parametrize("bad", [False, True], ids=["inside", "outside"])
@pytest.mark.parametrize("n", retidcases.SIZES)
def test_retid_routine_on_the_host_under_sanitizers(program, tmp_path, n, bad):
    """0, 1, 2, 65 and 300 records of 36 .. 200 bytes at each of the four byte skews, fields -1, 0, n_in - 1 and -- ``outside`` -- n_in,
    INT32_MIN and -2: the bytes (block_size, bytes 8 .. 23, everything from byte 28 on and the skew bytes included), the keys and the
    status equal the struct.pack_into translation; a record with a field outside is unchanged.  With and without keys."""
    n_in = 7
    table = retidcases.table(n_in)
    for skew in range(4):
        data, off, key = retidcases.stream(n, skew, n_in, bad=bad)
        for with_key in (True, False):
            want = retidcases.expected(data, off, table, key if with_key else None)
            got = retidcases.run_host(program, str(tmp_path / "case.bin"), data, off, table, key if with_key else None)
            assert np.array_equal(got[0], want[0]), (n, skew, with_key)
            assert (got[1] is None and want[1] is None) or np.array_equal(got[1], want[1])
            assert got[2] == want[2] == int(bad and n > 1), (n, skew, got[2], want[2])
        if bad and n > 1:                                       # the records with a field outside are there, and are as they were
            tid = np.asarray([int.from_bytes(data[int(o) + 4:int(o) + 8].tobytes(), "little", signed=True) for o in off])
            outside = np.flatnonzero((tid < -1) | (tid >= n_in))
            assert outside.size and all(np.array_equal(got[0][int(off[r]):int(off[r]) + 28], data[int(off[r]):int(off[r]) + 28]) for r in outside)


def test_retid_routine_one_reference_and_none(program, tmp_path):
    """n_in = 1: 0 is n_in - 1; n_in = 0: only -1 is inside."""
    data, off, key = retidcases.stream(65, 1, 1)
    table = np.asarray([4], np.int32)
    got, want = retidcases.run_host(program, str(tmp_path / "one.bin"), data, off, table, key), retidcases.expected(data, off, table, key)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] == 0 and (want[1] == 4).any()
    data, off, key = retidcases.stream(65, 3, 0)
    got = retidcases.run_host(program, str(tmp_path / "none.bin"), data, off, np.zeros(0, np.int32), key)
    assert np.array_equal(got[0], data) and np.array_equal(got[1], key) and got[2] == 0 and (key == -1).all()
