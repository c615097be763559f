"""Optional fields removed while a file is sorted (sort_bam's ``drop_tags`` / ``keep_tags``), the parts that need no GPU: the list
parser and its rules (sort.parse_tags, sort.tag_filter); the table (kernels.tags_bitmap) against tests/tagcases.py's, bit by bit; the
wave routines of svx_record_tags_measure / svx_record_tags_write (svision_amd/csrc/svx_recsort_core.hpp) in a stand-alone program
(tools/hostwave/tags_main.cpp) under AddressSanitizer and UBSan against tests/tagcases.py's walker, on every crafted stream, under
the drop list and under the complementary keep list; and the refusal of an input that is read as text (sort._open_all, which touches
no device for files)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from svision_amd import _lib, kernels, sort, sort_sources
from tests import htslike, mergecases as mc, tagcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFS = [("chr1", 1000), ("chr2", 2000)]
SQ = "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)


# ---- the lists ----
def test_good_lists():
    assert sort.parse_tags("fi,fp,ri,rp", "x") == ("fi", "fp", "ri", "rp") and sort.parse_tags(["RG", "X0"], "x") == ("RG", "X0")
    assert sort.parse_tags(("mv",), "x") == ("mv",) and sort.parse_tags("", "x") == () and sort.parse_tags([], "x") == ()
    assert sort.tag_filter(None, None, {}) is None
    assert sort.tag_filter("fi,fp", None, {}) == sort.TagFilter("drop", ("fi", "fp")) == sort_sources.TagFilter("drop", ("fi", "fp"))
    assert sort.tag_filter(None, ["RG", "NM"], {}) == sort.TagFilter("keep", ("RG", "NM"))
    assert sort.tag_filter(None, (), {}) == sort.TagFilter("keep", ())               # an empty keep list removes every field
    assert sort.tag_filter((), None, {}) is None                                      # an empty drop list removes nothing: off
    assert sort.tag_filter(None, "CG,NM", {}) == sort.TagFilter("keep", ("CG", "NM"))  # (naming CG in a keep list is fine: it is implied)


@pytest.mark.parametrize("bad", ["f", "f:", "fi:B", "1f", "fi,", ",fi", "fi, fp", "fiz", "f_", ["fi", "f"], ["fi", 7], [b"fi"], 7, {"fi"}])
def test_what_is_no_tag_list(bad):
    """A one-letter tag, a tag with ``:``, a digit first, an empty item, a blank, three letters, bytes, no list at all."""
    for kw in (dict(drop_tags=bad), dict(keep_tags=bad)):
        with pytest.raises(ValueError):
            sort.tag_filter(environ={}, **kw)


def test_a_repeat_cg_and_both_lists():
    with pytest.raises(ValueError, match="twice"):
        sort.tag_filter("fi,fp,fi", None, {})
    with pytest.raises(ValueError, match="twice"):
        sort.tag_filter(None, ["RG", "RG"], {})
    with pytest.raises(ValueError, match="CG"):
        sort.tag_filter("fi,CG", None, {})
    with pytest.raises(ValueError, match="exclude"):
        sort.tag_filter("fi", "RG", {})
    with pytest.raises(ValueError, match="exclude"):
        sort.tag_filter((), (), {})
    # sort_bam refuses such lists before it opens anything or asks for a device
    for kw in (dict(drop_tags="CG"), dict(drop_tags="fi", keep_tags="RG"), dict(keep_tags="R")):
        with pytest.raises(ValueError) as exc:
            sort.sort_bam("/nonexistent/in.bam", "/nonexistent/out.bam", **kw)
        assert not isinstance(exc.value, sort.SortWriteError)


def test_the_environment_variables():
    env = {"SVX_SORT_DROP_TAGS": "fi,fp,ri,rp"}
    assert sort.tag_filter(environ=env) == sort.TagFilter("drop", ("fi", "fp", "ri", "rp"))
    assert sort.tag_filter(environ={"SVX_SORT_KEEP_TAGS": "RG,NM,SA,MD"}) == sort.TagFilter("keep", ("RG", "NM", "SA", "MD"))
    assert sort.tag_filter(environ={"SVX_SORT_DROP_TAGS": "", "SVX_SORT_KEEP_TAGS": ""}) is None            # empty: unset
    assert sort.tag_filter(None, ["NM"], env) == sort.TagFilter("keep", ("NM",))                             # an argument wins
    assert sort.tag_filter((), None, env) is None
    with pytest.raises(ValueError, match="SVX_SORT_DROP_TAGS"):
        sort.tag_filter(environ={"SVX_SORT_DROP_TAGS": "fi:B:C"})
    with pytest.raises(ValueError, match="SVX_SORT_KEEP_TAGS"):
        sort.tag_filter(environ={"SVX_SORT_DROP_TAGS": "fi", "SVX_SORT_KEEP_TAGS": "RG"})
    with pytest.raises(ValueError, match="CG"):
        sort.tag_filter(environ={"SVX_SORT_DROP_TAGS": "CG"})


def test_the_command_line_refuses_a_bad_list_like_its_other_switches(monkeypatch, capsys):
    for argv, env, word in ((["--drop-tags", "f", "in.bam", "-o", "o.bam"], {}, "no tag"), (["--drop-tags", "fi", "--keep-tags", "RG", "in.bam", "-o", "o.bam"], {}, "exclude"),
                            (["in.bam", "-o", "o.bam"], {"SVX_SORT_KEEP_TAGS": "RG,RG"}, "SVX_SORT_KEEP_TAGS"), (["--drop-tags", "CG", "in.bam", "-o", "o.bam"], {}, "CG")):
        monkeypatch.delenv("SVX_SORT_DROP_TAGS", raising=False)
        monkeypatch.delenv("SVX_SORT_KEEP_TAGS", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with pytest.raises(SystemExit) as exc:
            sort.main(argv)
        assert exc.value.code == 2 and word in capsys.readouterr().err


def test_the_stage_the_switch_and_the_table():
    assert "tags" in sort.STAGES
    assert sort_sources.Opened("p", None, None, None, None, None).tags is None and sort_sources._Run(None, 1, 1, None, [], None).tags is None
    assert kernels.TAGS_TABLE_BYTES == tagcases.TABLE_BYTES
    for mode, tags in (("drop", ("fi", "fp")), ("drop", ("X0", "zz", "Az")), ("keep", ()), ("keep", ("RG", "NM")), ("keep", ("CG",)), ("drop", ())):
        got = kernels.tags_bitmap(tags, mode == "keep")
        assert got.dtype == np.dtype("<i4") and got.shape == (2048,) and np.array_equal(got, tagcases.bitmap(mode, tags))
        bits = np.unpackbits(got.view(np.uint8), bitorder="little")
        assert not bits[ord("C") | ord("G") << 8] and int(bits.sum()) == (len(tags) if mode == "drop" else 65536 - len(set(tags) | {"CG"}))
    assert np.array_equal(kernels.tags_bitmap([b"fi"], False), kernels.tags_bitmap(["fi"], False))
    with pytest.raises(_lib.SvxError):
        kernels.tags_bitmap(["CG"], False)
    with pytest.raises(_lib.SvxError):
        kernels.tags_bitmap(["fip"], False)


# ---- an input that is read as text ----
def _record(name):
    return htslike.encode_record(dict(tid=0, pos=5, qname=name, flag=0, mapq=9, cigar=[(8, "M")], seq="ACGTACGT", qual=None, tags=[("fi", "Z", "x")]))


def test_a_text_input_is_refused_under_the_switch_and_a_bam_keeps_its_room(tmp_path):
    """sort._open_all on files opens on the host.  SAM text under a filter: refused with its name, the switch and the way out; BAM
    inputs carry the filter, and their rooms -- the run's too -- stay the ISIZE sums."""
    a = mc.write_raw_bam(str(tmp_path / "a.bam"), SQ, REFS, [_record("a0")])
    c = mc.write_raw_bam(str(tmp_path / "c.bam"), SQ, REFS, [_record("c0"), _record("c1")])
    b = str(tmp_path / "b.sam")
    with open(b, "w") as f:
        f.write(SQ + "b0\t0\tchr1\t6\t9\t8M\t*\t0\t0\tACGTACGT\t*\tfi:Z:x\n")
    drop, keep = sort.TagFilter("drop", ("fi",)), sort.TagFilter("keep", ())
    run = lambda tags: sort_sources._Run(str(tmp_path / "out.bam"), 1, 1 << 20, None, [], None, False, False, tags)
    for paths in ([b], [a, b]):
        with pytest.raises(sort.SortWriteError) as exc:
            sort._open_all(paths, None, run(drop))
        msg = str(exc.value)
        assert "b.sam" in msg and "--drop-tags" in msg and "SVX_SORT_DROP_TAGS" in msg and "BAM" in msg and "a.bam" not in msg
    with pytest.raises(sort.SortWriteError, match="--keep-tags"):
        sort._open_all([b], None, run(keep))
    one = len(_record("a0"))
    ins = sort._open_all([a], None, run(drop))
    assert ins.opened[0].tags == drop and ins.merged.tags == drop and ins.merged.room == one
    ins = sort._open_all([a, c], None, run(keep))
    assert [o.tags for o in ins.opened] == [keep, keep] and [o.room for o in ins.opened] == [one, 2 * one] and ins.merged.room == 3 * one
    ins = sort._open_all([a, b], None, run(None))                   # off: as ever
    assert [o.tags for o in ins.opened] == [None, None] and ins.merged.room is None


# ---- the wave routines on the host ----
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_path_factory.mktemp("hostwave") / "tags_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", out, os.path.join(ROOT, "tools", "hostwave", "tags_main.cpp")])
    return out


def _check(program, path, records, drop, skew, status=None):
    """The stream at ``skew`` under the drop list and under the complementary keep list: the program agrees with the walker, and
    the two filters give the same bytes."""
    data, off = tagcases.place(records, skew)
    seen = []
    for mode, tags in tagcases.filters(records, drop):
        want, want_len, want_status = tagcases.expected(data, off, mode, tags)
        got, got_len, measured, written = tagcases.run_host(program, path, data, off, mode, tags)
        assert np.array_equal(got_len, want_len) and np.array_equal(got, want), (mode, tags)
        assert measured == written == want_status and (status is None or want_status == status)
        seen.append(want)
    assert np.array_equal(seen[0], seen[1])
    return want_len, off


@pytest.mark.parametrize("n", tagcases.COUNTS)
def test_tags_routines_on_the_host_record_counts(program, tmp_path, n):
    """1, 3, 4, 5 and 13 records at each of the four byte skews of the first one, the last one ending with the heap block."""
    for skew in range(4):
        new_len, off = _check(program, str(tmp_path / "case.bin"), tagcases.mixed(n, seed=skew), tagcases.DROP, skew, status=0)
        assert n < 12 or (new_len < np.diff(off)).any() and (new_len == np.diff(off)).any()


@pytest.mark.parametrize("case", tagcases.shape_cases(), ids=lambda c: c[0])
def test_tags_routines_on_the_host_shapes(program, tmp_path, case):
    name, records, drop = case
    bad = name.startswith("malformed")
    for skew in range(4):
        new_len, off = _check(program, str(tmp_path / "case.bin"), records, drop, skew, status=int(bad))
    if bad:                                                     # the neighbours were filtered, the bad record has its length
        which = 2 if "at the end" in name else 1
        assert new_len[which] == off[which + 1] - off[which] and all(new_len[r] < off[r + 1] - off[r] for r in range(3) if r != which)


def test_the_walker_on_literal_records():
    """The expectation itself, on records written out by hand: what tests/tagcases.walk gives is what the issue asks for."""
    fields = b"NMC\5" + b"fiBC\3\0\0\0abc" + b"RGZgrp\0" + b"fiZx\0" + b"MLBs\1\0\0\0\7\7" + b"mvH1F\0"
    rec = tagcases.record(fields, name=b"r\0", n_cigar=0, l_seq=0, seed=1)
    assert len(rec) == 38 + len(fields)
    new = tagcases.walk(rec, "drop", ("fi", "mv"))
    assert new[38:] == b"NMC\5RGZgrp\0MLBs\1\0\0\0\7\7" and new[4:38] == rec[4:38] and struct.unpack_from("<i", new)[0] == len(new) - 4
    assert tagcases.walk(rec, "keep", ("NM", "RG", "ML")) == new
    assert tagcases.walk(rec, "keep", ())[4:] == rec[4:38] and len(tagcases.walk(rec, "keep", ())) == 38
    assert tagcases.walk(rec, "drop", ("ZZ",)) == rec and tagcases.walk(rec, "drop", ("Fi", "iF", "bc")) == rec
    assert tagcases.walk(rec[:-1], "drop", ("fi",)) is None and tagcases.walk(rec + b"X", "drop", ("fi",)) is None
    assert all(tagcases.walk(tagcases.malformed(kind), "keep", ()) is None for kind in tagcases.MALFORMED)
    cg = tagcases.cg_record()
    assert tagcases.walk(cg, "keep", ()) == tagcases.walk(cg, "drop", ("NM",)) and b"CGBI" in tagcases.walk(cg, "keep", ("XD",))
    assert tagcases.complement([rec], ("fi", "mv")) == ("NM", "RG", "ML")
