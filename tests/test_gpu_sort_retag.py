"""sort_bam(..., retag=True) on several inputs whose @RG / @PG IDs collide (svision_amd/sort.py, sort_sources._retag,
svx_record_retag_measure / svx_record_retag_write): the two files must be, byte for byte, those that sort_bam writes for ONE unsorted
BAM that holds the merged header -- written out literally here -- and the inputs' records one input after the other, the later
inputs' records rewritten by tests/retagcases.py's walker.  In one piece, in spans, in several ranges an input, with a renumbered
dictionary; nothing to rename; the refusals."""
import os

import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from tests import helpers, mergecases as mc, retagcases as rc, sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 240                                                         # records an input

RG_A, RG_B, RG_C, RG_SOLO = "@RG\tID:1\tSM:s\tPU:cell_a\n", "@RG\tID:1\tSM:s\tPU:cell_b\n", "@RG\tID:1\tSM:s\tPU:cell_c\n", "@RG\tID:solo\tSM:s\n"
PG_A, PG_B = "@PG\tID:aln\tPN:aln\tCL:aln a.fq\n", "@PG\tID:aln\tPN:aln\tCL:aln b.fq\n"
HD = "@HD\tVN:1.6\tSO:unsorted\n"


def _pair(path):
    return open(path, "rb").read(), open(path + ".bai", "rb").read()


def _sorted(inputs, out, **kw):
    from svision_amd import sort
    stats = {}
    assert sort.sort_bam(inputs, out, device=DEV, stats=stats, **kw) == out
    assert not [n for n in os.listdir(os.path.dirname(out)) if n.endswith(".tmp")]
    return _pair(out), stats


def _tagged(records, rg):
    """Every record with tags behind its own, in turn: RG then PG, PG then RG with a long string between, RG alone, none, a read
    group that is not the colliding one."""
    long_z = rc.z("MM", b"C+m,1,5,0;" * 30)
    kinds = (rc.z("RG", rg) + rc.z("PG", b"aln"), rc.z("PG", b"aln") + long_z + rc.z("RG", rg), rc.z("RG", rg), b"", rc.z("RG", b"solo") + rc.fixed("NM", "i", 3))
    return [rc.with_fields(r, kinds[i % len(kinds)]) for i, r in enumerate(records)]


@pytest.fixture(scope="module")
def colliding(tmp_path_factory):
    """Three BAM inputs: the 2nd brings @RG 1 and @PG aln on other lines than the 1st and a read group of its own, the 3rd @RG 1 on a
    third line and the 1st input's @PG line.  -> (directory, the inputs, the 2nd with its dictionary turned round, the one file,
    its records, the references, the records the walker changed)."""
    d = str(tmp_path_factory.mktemp("sort_retag"))
    path, _sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), d, 47)
    _text, refs, records = mc.raw_bam(path)
    assert len(records) >= 3 * N and len(refs) == 2
    parts = [_tagged(records[i * N:(i + 1) * N], b"1") for i in range(3)]
    sq = mc.sq(refs)
    a = mc.write_raw_bam(os.path.join(d, "a.bam"), HD + sq + RG_A + PG_A, refs, parts[0])
    b = mc.write_raw_bam(os.path.join(d, "b.bam"), HD + sq + RG_B + RG_SOLO + PG_B, refs, parts[1])
    b_turned = mc.write_raw_bam(os.path.join(d, "b_turned.bam"), HD + mc.sq(refs[::-1]) + RG_B + RG_SOLO + PG_B, refs[::-1],
                                [mc.renumbered(r, refs, refs[::-1]) for r in parts[1]])
    c = mc.write_raw_bam(os.path.join(d, "c.bam"), HD + sq + RG_C + PG_A, refs, parts[2])
    # the merged header, by hand: a later input's new line goes behind the last line of its type
    text = (HD + sq + RG_A + "@RG\tID:1-2\tSM:s\tPU:cell_b\n" + RG_SOLO + "@RG\tID:1-3\tSM:s\tPU:cell_c\n" + PG_A + "@PG\tID:aln-2\tPN:aln\tCL:aln b.fq\n")
    new_b = [rc.walk(r, {("RG", b"1"): b"1-2", ("PG", b"aln"): b"aln-2"}) for r in parts[1]]
    new_c = [rc.walk(r, {("RG", b"1"): b"1-3"}) for r in parts[2]]
    assert None not in new_b + new_c
    changed = sum(x != y for x, y in zip(parts[1] + parts[2], new_b + new_c))
    assert changed == 2 * (N - 2 * (N // 5))                     # every record but those without tags and those of ``solo``
    one_records = parts[0] + new_b + new_c
    one = mc.write_raw_bam(os.path.join(d, "one.bam"), text, refs, one_records)
    return d, [a, b, c], b_turned, one, one_records, refs, changed


def test_colliding_ids_are_renamed_and_the_records_follow(colliding, tmp_path):
    from svision_amd import sort
    _d, inputs, b_turned, one, one_records, refs, changed = colliding
    want, one_stats = _sorted(one, str(tmp_path / "one.bam"))
    got, stats = _sorted(inputs, str(tmp_path / "merged.bam"), retag=True)
    assert got == want
    assert stats["inputs"] == 3 and stats["retag_inputs"] == 2 and stats["retag_records"] == changed and stats["retid_inputs"] == 0
    assert stats["seconds"]["retag"] > 0 and set(stats["seconds"]) == set(sort.STAGES) and stats["spans"] == 1
    assert stats["input_records"] == [N, N, N] and one_stats["retag_inputs"] == 0 and one_stats["retag_records"] == 0 and one_stats["seconds"]["retag"] == 0.0
    assert stats["stream_bytes"] == sum(len(r) for r in one_records) + 4
    # the written file: every RG value names an @RG line of its header, every PG value a @PG line
    text, out_refs, records = mc.raw_bam(str(tmp_path / "merged.bam"))
    ids = {kind: {f[3:] for l in text.split("\n") if l.startswith(kind + "\t") for f in l.split("\t") if f.startswith("ID:")} for kind in ("@RG", "@PG")}
    assert out_refs == refs and ids == {"@RG": {"1", "1-2", "solo", "1-3"}, "@PG": {"aln", "aln-2"}}
    values = {tag: [v.decode() for r in records for v in rc.z_values(r, tag)] for tag in ("RG", "PG")}
    assert set(values["RG"]) == ids["@RG"] and set(values["PG"]) == ids["@PG"] and len(values["RG"]) == 3 * (N - N // 5)
    assert sorted(records) == sorted(one_records)
    # the environment turns it on where the argument says nothing
    old = os.environ.get("SVX_SORT_RETAG")
    os.environ["SVX_SORT_RETAG"] = "1"
    try:
        assert _sorted(inputs, str(tmp_path / "env.bam"))[0] == want
    finally:
        os.environ.pop("SVX_SORT_RETAG") if old is None else os.environ.__setitem__("SVX_SORT_RETAG", old)


def test_in_spans_in_ranges_and_with_a_renumbered_input(colliding, tmp_path):
    _d, inputs, b_turned, one, one_records, _refs, changed = colliding
    want = _sorted(one, str(tmp_path / "one.bam"))[0]
    record_bytes = sum(len(r) for r in one_records)
    got, stats = _sorted(inputs, str(tmp_path / "spans.bam"), retag=True, memory_bytes=record_bytes // 4)
    assert got == want and stats["spans"] >= 3 and stats["span_range_reads"] >= stats["spans"] and stats["retag_records"] == changed
    got, stats = _sorted(inputs, str(tmp_path / "ranges.bam"), retag=True, range_bytes=1 << 13)
    assert got == want and stats["ranges"] >= 9 and stats["spans"] == 1 and stats["retag_records"] == changed
    turned = [inputs[0], b_turned, inputs[2]]
    got, stats = _sorted(turned, str(tmp_path / "turned.bam"), retag=True)
    assert got == want and stats["retid_inputs"] == 1 and stats["retag_inputs"] == 2
    got, stats = _sorted(turned, str(tmp_path / "all.bam"), retag=True, memory_bytes=record_bytes // 4, range_bytes=1 << 13)
    assert got == want and stats["spans"] >= 3 and stats["ranges"] >= 9 and stats["retid_inputs"] == 1 and stats["retag_records"] == changed


def test_nothing_to_rename_is_the_run_it_was(colliding, tmp_path):
    d, inputs, _b_turned, _one, _one_records, refs, _changed = colliding
    _text, _refs, records = mc.raw_bam(inputs[1])
    distinct = mc.write_raw_bam(os.path.join(d, "distinct.bam"), HD + mc.sq(refs) + "@RG\tID:2\tSM:s\tPU:cell_b\n" + RG_SOLO + PG_A, refs, records)
    plain, plain_stats = _sorted([inputs[0], distinct], str(tmp_path / "plain.bam"), retag=False)
    got, stats = _sorted([inputs[0], distinct], str(tmp_path / "retag.bam"), retag=True)
    assert got == plain
    assert stats["retag_inputs"] == 0 and stats["retag_records"] == 0 and stats["seconds"]["retag"] == 0.0
    assert plain_stats["retag_inputs"] == 0 and plain_stats["seconds"]["retag"] == 0.0
    same = lambda st: {k: v for k, v in st.items() if k not in ("seconds", "memory_bytes")}
    assert same(stats) == same(plain_stats)


def test_refusals_leave_nothing_behind(colliding, tmp_path):
    from svision_amd import sort
    _d, inputs, _b_turned, _one, _one_records, refs, _changed = colliding
    src, out_dir = str(tmp_path / "in"), str(tmp_path / "out")
    os.makedirs(src)
    os.makedirs(out_dir)
    text = os.path.join(src, "text.sam")
    with open(text, "w") as f:
        f.write(HD + mc.sq(refs) + RG_B + "t0\t0\t%s\t6\t9\t8M\t*\t0\t0\tACGTACGT\t*\tRG:Z:1\n" % refs[0][0])
    with pytest.raises(sort.SortWriteError) as exc:
        sort.sort_bam([inputs[0], text], os.path.join(out_dir, "never.bam"), device=DEV, retag=True)
    assert "text.sam" in str(exc.value) and "1-2" in str(exc.value) and "first" in str(exc.value), str(exc.value)
    assert os.listdir(out_dir) == []
    for second in (text, inputs[1]):                            # without the switch: refused as ever
        with pytest.raises(sort.SortWriteError) as exc:
            sort.sort_bam([inputs[0], second], os.path.join(out_dir, "never.bam"), device=DEV, retag=False)
        assert "RG:Z" in str(exc.value) and "a.bam" in str(exc.value) and os.path.basename(second) in str(exc.value)
        assert os.listdir(out_dir) == []
    # the text listed first keeps the ID, and the BAM behind it is rewritten
    got, stats = _sorted([text, inputs[0]], os.path.join(out_dir, "first.bam"), retag=True)
    assert stats["retag_inputs"] == 1 and stats["input_records"] == [1, N] and stats["retag_records"] == N - 2 * (N // 5)
    values = [v for r in mc.raw_bam(os.path.join(out_dir, "first.bam"))[2] for v in rc.z_values(r, "RG")]
    assert values.count(b"1") == 1 and values.count(b"1-2") == N - 2 * (N // 5) and values.count(b"solo") == N // 5
