"""Colliding @RG / @PG IDs of several inputs renamed and the records' tags rewritten (sort_bam's ``retag``), the parts that need no
GPU: the header rules (sort_header.merge_headers(retag=True)) on literal texts; the wave routines of svx_record_retag_measure /
svx_record_retag_write (svision_amd/csrc/svx_recsort_core.hpp) in a stand-alone program (tools/hostwave/retag_main.cpp) under
AddressSanitizer and UBSan against tests/retagcases.py's walker, on every crafted stream; and the refusal of an input that is read as
text (sort._open_all, which touches no device for files)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from svision_amd import kernels, sort, sort_sources
from tests import htslike, mergecases as mc, retagcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = [("chr1", 1000), ("chr2", 2000)]
SQ = "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)


def _part(name, text, refs=REFS):
    return (name, text, [r[0] for r in refs], [r[1] for r in refs])


# ---- the header rules ----
def test_a_colliding_rg_is_renamed_and_the_first_input_keeps_the_id():
    a = SQ + "@RG\tID:1\tSM:s\tPU:cell_a\n"
    b = SQ + "@RG\tID:1\tSM:s\tPU:cell_b\n@RG\tID:2\tSM:s\tPU:cell_b2\n"
    c = SQ + "@RG\tID:1\tSM:s\tPU:cell_c\n@RG\tID:2\tSM:s\tPU:cell_b2\n"
    m = sort.merge_headers([_part("a.bam", a), _part("b.bam", b), _part("c.bam", c)], retag=True)
    assert m.text == ("@HD\tVN:1.6\tSO:coordinate\n" + SQ + "@RG\tID:1\tSM:s\tPU:cell_a\n@RG\tID:1-2\tSM:s\tPU:cell_b\n@RG\tID:2\tSM:s\tPU:cell_b2\n"
                      "@RG\tID:1-3\tSM:s\tPU:cell_c\n")
    assert m.renames == [{}, {("RG", b"1"): b"1-2"}, {("RG", b"1"): b"1-3"}]
    # without the switch: refused as ever, and the message names the switch
    with pytest.raises(sort.SortWriteError) as exc:
        sort.merge_headers([_part("a.bam", a), _part("b.bam", b)])
    msg = str(exc.value)
    assert "a.bam" in msg and "b.bam" in msg and "RG:Z" in msg and "which this tool does not do" in msg and "--retag" in msg and "SVX_SORT_RETAG" in msg


def test_a_suffix_that_is_taken_is_refused_with_both_names():
    a = SQ + "@RG\tID:1\tSM:s\tPU:cell_a\n@RG\tID:1-2\tSM:s\tPU:odd\n"
    b = SQ + "@RG\tID:1\tSM:s\tPU:cell_b\n"
    with pytest.raises(sort.SortWriteError) as exc:
        sort.merge_headers([_part("/d/a.bam", a), _part("/d/b.bam", b)], retag=True)
    assert "/d/a.bam" in str(exc.value) and "/d/b.bam" in str(exc.value) and "1-2" in str(exc.value)
    # taken by a line of the later input itself
    a = SQ + "@RG\tID:1\tSM:s\tPU:cell_a\n"
    b = SQ + "@RG\tID:1\tSM:s\tPU:cell_b\n@RG\tID:1-2\tSM:s\tPU:own\n"
    with pytest.raises(sort.SortWriteError) as exc:
        sort.merge_headers([_part("/d/a.bam", a), _part("/d/b.bam", b)], retag=True)
    assert "/d/a.bam" in str(exc.value) and "/d/b.bam" in str(exc.value) and "1-2" in str(exc.value)


def test_an_identical_line_appears_once_and_renames_nothing():
    a = SQ + "@RG\tID:rg\tSM:one\n@PG\tID:aln\tPN:aln\tCL:aln x\n"
    m = sort.merge_headers([_part("a", a), _part("b", a), _part("c", SQ + "@RG\tID:rg\tSM:one\n@RG\tID:rg2\tSM:one\n")], retag=True)
    assert m.text == "@HD\tVN:1.6\tSO:coordinate\n" + SQ + "@RG\tID:rg\tSM:one\n@RG\tID:rg2\tSM:one\n@PG\tID:aln\tPN:aln\tCL:aln x\n"
    assert m.renames == [{}, {}, {}]


def test_pp_follows_a_pg_rename_and_the_tables_hold_it():
    a = SQ + "@PG\tID:minimap2\tPN:minimap2\tCL:minimap2 -a ref.fa one.fq\n@PG\tID:samtools\tPN:samtools\tPP:minimap2\tCL:samtools view -b\n"
    b = SQ + "@RG\tID:1\tSM:s\n@PG\tID:minimap2\tPN:minimap2\tCL:minimap2 -a ref.fa two.fq\n@PG\tID:samtools\tPN:samtools\tPP:minimap2\tCL:samtools view -b\n" \
        "@PG\tID:other\tPN:other\n"
    want = ("@HD\tVN:1.6\tSO:coordinate\n" + SQ
            + "@PG\tID:minimap2\tPN:minimap2\tCL:minimap2 -a ref.fa one.fq\n@PG\tID:samtools\tPN:samtools\tPP:minimap2\tCL:samtools view -b\n"
            + "@PG\tID:minimap2-2\tPN:minimap2\tCL:minimap2 -a ref.fa two.fq\n@PG\tID:samtools-2\tPN:samtools\tPP:minimap2-2\tCL:samtools view -b\n"
            + "@PG\tID:other\tPN:other\n"
            + "@RG\tID:1\tSM:s\n")                            # (no @RG line so far: a later input's goes to the end)
    m = sort.merge_headers([_part("a", a), _part("b", b)], retag=True)
    assert m.text == want
    assert m.renames == [{}, {("PG", b"minimap2"): b"minimap2-2", ("PG", b"samtools"): b"samtools-2"}]
    # without the switch: today's text, the rename stays in the header, and every table is empty
    off = sort.merge_headers([_part("a", a), _part("b", b)])
    assert off.text == want and off.renames == [{}, {}]
    assert sort.merge_headers([_part("a", a)]).renames == [{}] and sort.merge_headers([_part("a", a)], retag=True).renames == [{}]
    assert sort.MergedHeader("t", [], [], []).renames == ()         # (the field has a default: earlier callers construct four)


def test_the_stage_the_switch_and_the_table():
    assert "retag" in sort.STAGES
    assert sort_sources.Opened("p", None, None, None, None, None).retag is None and sort_sources._Run(None, 1, 1, None, [], None).retag is False
    flat, off, m = kernels.retag_pack(retagcases.RENAMES)
    want_flat, want_off = retagcases.pack(retagcases.RENAMES)
    assert m == 3 and np.array_equal(flat, want_flat) and np.array_equal(off, want_off) and off.dtype == np.int32
    assert kernels.retag_pack({})[2] == 0
    from svision_amd import _lib
    with pytest.raises(_lib.SvxError):
        kernels.retag_pack({("RGX", b"a"): b"b"})
    with pytest.raises(_lib.SvxError):
        kernels.retag_pack({("RG", b"a\0"): b"b"})


# ---- an input that is read as text ----
def _record(name, rg):
    return htslike.encode_record(dict(tid=0, pos=5, qname=name, flag=0, mapq=9, cigar=[(8, "M")], seq="ACGTACGT", qual=None, tags=[("RG", "Z", rg)]))


def test_a_text_input_that_needs_a_rename_is_refused(tmp_path):
    """sort._open_all on files opens and merges on the host.  A SAM part whose @RG collides: refused under the switch, with its name,
    the ID and the way out; listed first it keeps the ID and the BAM part takes the table, its run's room unknown, its own kept."""
    a = mc.write_raw_bam(str(tmp_path / "a.bam"), SQ + "@RG\tID:1\tPU:a\n", REFS, [_record("a0", "1")])
    with open(str(tmp_path / "b.sam"), "w") as f:
        f.write(SQ + "@RG\tID:1\tPU:b\n" + "b0\t0\tchr1\t6\t9\t8M\t*\t0\t0\tACGTACGT\t*\tRG:Z:1\n")
    b = str(tmp_path / "b.sam")
    run = lambda retag: sort_sources._Run(str(tmp_path / "out.bam"), 1, 1 << 20, None, [], None, False, retag)
    with pytest.raises(sort.SortWriteError) as exc:
        sort._open_all([a, b], None, run(True))
    msg = str(exc.value)
    assert "b.sam" in msg and "@RG ID 1" in msg and "1-2" in msg and "first" in msg and "a.bam" not in msg
    ins = sort._open_all([b, a], None, run(True))
    assert ins.opened[0].retag is None and ins.opened[1].retag == {("RG", b"1"): b"1-2"}
    assert ins.merged.room is None and ins.opened[1].room == len(_record("a0", "1"))
    with pytest.raises(sort.SortWriteError, match="RG:Z"):
        sort._open_all([a, b], None, run(False))
    # nothing collides: no table, and the BAM's room is the run's business as before
    c = mc.write_raw_bam(str(tmp_path / "c.bam"), SQ + "@RG\tID:3\tPU:c\n", REFS, [_record("c0", "3")])
    ins = sort._open_all([a, c], None, run(True))
    assert [o.retag for o in ins.opened] == [None, None] and ins.merged.room == 2 * len(_record("a0", "1"))


# ---- the wave routines on the host ----
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_path_factory.mktemp("hostwave") / "retag_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", out, os.path.join(ROOT, "tools", "hostwave", "retag_main.cpp")])
    return out


def _check(program, path, records, renames, skew, status=None):
    data, off = retagcases.place(records, skew)
    want, want_len, want_status = retagcases.expected(data, off, renames)
    got, got_len, measured, written = retagcases.run_host(program, path, data, off, renames)
    assert np.array_equal(got_len, want_len) and np.array_equal(got, want)
    assert measured == written == want_status and (status is None or want_status == status)
    return want_len, off


@pytest.mark.parametrize("n", retagcases.COUNTS)
def test_retag_routines_on_the_host_record_counts(program, tmp_path, n):
    """0, 1, 63, 64, 65 and 257 records at each of the four byte skews of the first one, the last one ending with the heap block."""
    for skew in range(4):
        records = retagcases.mixed(n, seed=skew)
        new_len, off = _check(program, str(tmp_path / "case.bin"), records, retagcases.RENAMES, skew, status=0)
        assert n < 12 or (new_len > np.diff(off)).any() and (new_len < np.diff(off)).any() and (new_len == np.diff(off)).any()


@pytest.mark.parametrize("case", retagcases.shape_cases(), ids=lambda c: c[0])
def test_retag_routines_on_the_host_shapes(program, tmp_path, case):
    name, records, renames = case
    bad = name.startswith("malformed")
    for skew in (0, 3) if len(b"".join(records)) > 1 << 20 else range(4):
        new_len, off = _check(program, str(tmp_path / "case.bin"), records, renames, skew, status=int(bad))
    if bad:                                                     # the neighbours were rewritten, the bad record has its length
        which = 2 if "at the end" in name else 1
        assert new_len[which] == off[which + 1] - off[which] and all(new_len[r] != off[r + 1] - off[r] for r in range(3) if r != which)


def test_the_walker_on_literal_records():
    """The expectation itself, on records written out by hand: what tests/retagcases.walk gives is what the issue asks for."""
    rec = retagcases.record(b"RGZgrp1\0NMC\5PGZminimap2.long\0", name=b"r\0", n_cigar=0, l_seq=0, seed=1)
    new = retagcases.walk(rec, retagcases.RENAMES)
    assert new[36 + 2:] == b"RGZgrp1-2\0NMC\5PGZmm\0" and len(new) == len(rec) + 2 - 11 and new[4:38] == rec[4:38]
    assert int.from_bytes(new[:4], "little") == len(new) - 4
    assert retagcases.walk(rec, retagcases.ONLY_RG)[38:] == b"RGZgrp1-2\0NMC\5PGZminimap2.long\0"
    assert retagcases.walk(rec, {("RG", b"grp"): b"no", ("RG", b"grp12"): b"no"}) == rec
    assert retagcases.walk(rec[:-1], retagcases.RENAMES) is None and retagcases.walk(rec + b"X", retagcases.RENAMES) is None
    assert all(retagcases.walk(retagcases.malformed(kind), retagcases.RENAMES) is None for kind in retagcases.MALFORMED)
