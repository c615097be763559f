"""sort_bam on SEVERAL inputs (svision_amd/sort.py: merge_headers, svx_record_retid): the two files must be, byte for byte, those that
sort_bam writes for ONE unsorted BAM that holds the merged header and the inputs' records one input after the other, every reference
index in the merged numbering.  That one file is written here: the inputs' record bytes re-packed with ``struct`` under a header text
assembled by hand (tests/mergecases.py).  Same and different dictionaries, ties across inputs, SAM text among the inputs, in spans,
one input, the refusals and the command lines."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from svision_amd.io import bam
from tests import helpers, htslike, mergecases as mc, samtext, sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = ("extra_contig", 4242)


def _read(path):
    return open(path, "rb").read()


def _pair(path):
    return _read(path), _read(path + ".bai")


def _sorted(inputs, out, **kw):
    from svision_amd import sort
    stats = {}
    assert sort.sort_bam(inputs, out, device=DEV, stats=stats, **kw) == out
    assert not [n for n in os.listdir(os.path.dirname(out)) if n.endswith(".tmp")]
    return _pair(out), stats


@pytest.fixture(scope="module")
def shuffled(tmp_path_factory):
    """collect_small's records in a seeded random order: (directory, the shuffled file, the stably sorted file, header text, references,
    the records' bytes in the shuffled file's order)."""
    d = str(tmp_path_factory.mktemp("sort_merge"))
    path, sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), d, 31)
    text, refs, records = mc.raw_bam(path)
    assert len(records) > 1000 and [r[0] for r in refs] == ["chrA", "chrB"]
    return d, path, sorted_path, text, refs, records


# ---- 1. the same header, three parts ----
@pytest.fixture(scope="module")
def same_header(shuffled):
    d, _path, _sorted_path, text, refs, records = shuffled
    parts = [mc.write_raw_bam(os.path.join(d, "same.%d.bam" % i), text, refs, records[i::3]) for i in range(3)]
    one = mc.write_raw_bam(os.path.join(d, "same.one.bam"), text, refs, records[0::3] + records[1::3] + records[2::3])
    return parts, one


@pytest.mark.parametrize("tables", ["fixed", "dynamic"])
def test_same_header_three_parts(same_header, tmp_path, tables):
    from svision_amd import sort
    parts, one = same_header
    want, one_stats = _sorted(one, str(tmp_path / "one.bam"), tables=tables)
    got, stats = _sorted(parts, str(tmp_path / "merged.bam"), tables=tables)
    assert got == want
    assert stats["inputs"] == 3 and stats["retid_inputs"] == 0 and sum(stats["input_records"]) == stats["records"] == one_stats["records"]
    assert stats["input_records"] == [497, 497, 497] and stats["seconds"]["retid"] == 0.0 and set(stats["seconds"]) == set(sort.STAGES)
    assert stats["ranges"] == 3 and sum(stats["range_records"]) == stats["records"] and stats["spans"] == 1
    assert one_stats["inputs"] == 1 and one_stats["retid_inputs"] == 0 and one_stats["input_records"] == [one_stats["records"]]
    # a tuple is a list; small ranges and chunks: the same files
    got, stats = _sorted(tuple(parts), str(tmp_path / "small.bam"), tables=tables, range_bytes=1 << 14, chunk_bytes=2 * htslike.BLOCK)
    assert got == want and stats["ranges"] > 6 and stats["chunks"] > 3


# ---- 2. different dictionaries ----
@pytest.fixture(scope="module")
def dictionaries(shuffled):
    """Part A lists chrA chrB, part B chrB chrA and a contig nobody uses, part C only chrB -- its records lie there.  Every fifth
    record of A and B gets a mate on the other reference, every part three records without a reference.  -> (the parts, the one
    file in the merged numbering, its records, the merged references)."""
    d, _path, _sorted_path, text, refs, records = shuffled
    own = {"a": refs, "b": [refs[1], refs[0], EXTRA], "c": [refs[1]]}
    merged = refs + [EXTRA]
    dealt = {"a": [], "b": [], "c": []}
    for i, rec in enumerate(records):
        part = "abc"[i % 3]
        if part == "c" and mc.tid(rec) != 1:
            part = "a"
        if part != "c" and i % 5 == 0:
            rec = mc.with_refs(rec, mc.tid(rec), 1 - mc.tid(rec), 777 + i)
        elif i % 7 == 0:
            rec = mc.with_refs(rec, mc.tid(rec), mc.tid(rec), 55 + i)
        dealt[part].append(rec)
    for part in "abc":
        dealt[part][3:3] = [mc.unmapped("%s_unmapped_%d" % (part, j)) for j in range(3)]
    body = "@PG\tID:aligner\tPN:aligner\tCL:aligner %s.fq\n@CO\tpart %s\n@CO\tshared comment\n"
    paths = [mc.write_raw_bam(os.path.join(d, "dict.%s.bam" % p), "@HD\tVN:1.6\tSO:unsorted\n" + mc.sq(own[p]) + body % (p, p), own[p],
                              [mc.renumbered(r, refs, own[p]) for r in dealt[p]]) for p in "abc"]
    # the merged header, by hand: A's lines; B's new reference behind the @SQ lines, its @PG renamed behind the @PG lines, its new @CO
    # behind the @CO lines; then C's
    text = ("@HD\tVN:1.6\tSO:unsorted\n" + mc.sq(merged)
            + "@PG\tID:aligner\tPN:aligner\tCL:aligner a.fq\n@PG\tID:aligner-2\tPN:aligner\tCL:aligner b.fq\n@PG\tID:aligner-3\tPN:aligner\tCL:aligner c.fq\n"
            + "@CO\tpart a\n@CO\tshared comment\n@CO\tpart b\n@CO\tpart c\n")
    one_records = dealt["a"] + dealt["b"] + dealt["c"]
    one = mc.write_raw_bam(os.path.join(d, "dict.one.bam"), text, merged, one_records)
    assert len(dealt["c"]) > 100 and all(mc.tid(r) in (1, -1) for r in dealt["c"])
    return paths, one, one_records, merged


@pytest.mark.parametrize("tables", ["fixed", "dynamic"])
def test_different_dictionaries(dictionaries, tmp_path, tables):
    paths, one, one_records, merged = dictionaries
    want, _one_stats = _sorted(one, str(tmp_path / "one.bam"), tables=tables)
    got, stats = _sorted(paths, str(tmp_path / "merged.bam"), tables=tables)
    assert got == want
    assert stats["inputs"] == 3 and stats["retid_inputs"] == 2 and sum(stats["input_records"]) == len(one_records) and stats["seconds"]["retid"] > 0
    if tables == "dynamic":
        return
    # the written file, read back: the header, and the records of the one file in sortcases.order
    out = str(tmp_path / "merged.bam")
    text, refs, records = mc.raw_bam(out)
    assert refs == merged and text.startswith("@HD\tVN:1.6\tSO:coordinate\n" + mc.sq(merged) + "@PG\tID:aligner\t")
    tid, pos = np.asarray([mc.tid(r) for r in one_records]), np.asarray([mc.pos(r) for r in one_records])
    order = sortcases.order(tid, pos, len(merged))
    assert records == [one_records[i] for i in order]
    # mates on another reference keep pointing at it
    cross = [r for r in records if mc.next_tid(r) >= 0 and mc.next_tid(r) != mc.tid(r)]
    assert len(cross) > 100 and all(mc.next_tid(r) == 1 - mc.tid(r) for r in cross) and {mc.tid(r) for r in cross} == {0, 1}
    # the host reader and the device decoder
    from svision_amd import ingest_gpu
    whole, head = bam.read_bam(out), bam.read_bam_header(out)
    assert whole.sort_order == "coordinate" and list(head.references) == [r[0] for r in merged] and list(head.lengths) == [r[1] for r in merged]
    assert np.array_equal(whole.tid, tid[order]) and np.array_equal(whole.pos, pos[order])
    assert np.array_equal(whole.flag, np.asarray([mc.flag(one_records[i]) for i in order]))
    assert [whole.names[int(i)] for i in whole.name_id[-3:]] == ["c_unmapped_0", "c_unmapped_1", "c_unmapped_2"]
    dec = ingest_gpu.DeviceDecoder(out, out + ".bai", head.references, head.lengths, head.header_text, DEV, threads=3)
    tids = [0, 1]
    assert dec.usable(tids)
    seen = 0
    for finish, _arrays in dec.parts_pipelined(tids):
        tb = finish()
        host = whole.subset(np.flatnonzero(whole.tid == int(tb.tid[0])))
        for fld in ("tid", "pos", "flag", "mapq", "l_seq"):
            assert np.array_equal(getattr(tb, fld), getattr(host, fld)), fld
        seen += len(host)
    assert seen == int((tid >= 0).sum())


# ---- 3. ties across inputs ----
def test_ties_come_out_in_list_order(tmp_path):
    refs = [("chrA", 5000), ("chrB", 6000)]

    def part(name, own):
        at = {r[0]: i for i, r in enumerate(own)}
        recs = [htslike.encode_record(dict(tid=at[ref], pos=p, qname="%s_%d" % (name, j), flag=0, mapq=9, cigar=[(8, "M")], seq="ACGTACGT", qual=None))
                for j, (ref, p) in enumerate((("chrB", 40), ("chrA", 100), ("chrA", 100), ("chrB", 40), ("chrA", 7)))]
        return mc.write_raw_bam(str(tmp_path / (name + ".bam")), "@HD\tVN:1.6\n" + mc.sq(own), own, recs)
    x, y, z = part("x", refs), part("y", refs[::-1]), part("z", refs)

    def names(inputs):
        out = str(tmp_path / "ties.bam")
        _sorted(inputs, out)
        return [mc.qname(r) for r in mc.raw_bam(out)[2]]
    by_part = lambda order: [["%s_4" % p for p in order], ["%s_%d" % (p, j) for p in order for j in (1, 2)], ["%s_%d" % (p, j) for p in order for j in (0, 3)]]
    assert names([x, y, z]) == sum(by_part("xyz"), [])
    assert names([z, x, y]) == sum(by_part("zxy"), [])
    # y first: ITS dictionary opens the merged one, chrB comes first
    got = names([y, x, z])
    assert got == sum([by_part("yxz")[2], by_part("yxz")[0], by_part("yxz")[1]], [])


# ---- 4. SAM text among the inputs ----
@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """Three parts of collect_small's records as dicts: every part as a BAM of tests/htslike.py, the second also as SAM text under
    the same header, the third as SAM text without any header."""
    d = str(tmp_path_factory.mktemp("sort_mixed"))
    table = bam.read_bam(os.path.join(helpers.GOLDEN, "collect_small.bam"), with_seq=True)
    rng = np.random.default_rng(8)
    recs = samtext.records_of_table(table, rng, tags=True)
    recs = [recs[i] for i in rng.permutation(len(recs))]
    refs = list(zip(table.references, table.lengths))
    own = [refs, refs[::-1], refs]
    out = dict(bam=[], sam=[], n=len(recs), dir=d)
    for i in range(3):
        mine = [dict(r, tid=own[i].index(refs[r["tid"]])) for r in recs[i::3]]
        text = samtext.header_text(own[i])
        p = os.path.join(d, "part%d.bam" % i)
        htslike.write_bam(p, own[i], [samtext.for_htslike(r) for r in mine], level=1, policy="stream", header_text=text, index=False)
        out["bam"].append(p)
        s = os.path.join(d, "part%d.sam" % i)
        with open(s, "wb") as f:
            f.write(samtext.text(own[i], mine, header="" if i == 2 else text))
        out["sam"].append(s)
    return out


@pytest.mark.parametrize("tables", ["fixed", "dynamic"])
def test_sam_text_among_the_inputs(mixed, tmp_path, tables):
    want, bam_stats = _sorted(mixed["bam"], str(tmp_path / "all_bam.bam"), tables=tables)
    assert bam_stats["retid_inputs"] == 1 and bam_stats["records"] == mixed["n"] and "input" not in bam_stats and "host_lines" not in bam_stats
    inputs = [mixed["bam"][0], mixed["sam"][1], mixed["sam"][2]]
    got, stats = _sorted(inputs, str(tmp_path / "mixed.bam"), tables=tables)
    assert got == want
    assert stats["inputs"] == 3 and stats["retid_inputs"] == 0 and stats["input_records"] == bam_stats["input_records"] and stats["host_lines"] == 0
    assert "input" not in stats and stats["spans"] == 1 and stats["stream_bytes"] == bam_stats["stream_bytes"]
    if tables == "fixed":
        # the BAM part behind the text, and renumbered: read a second time like the first; every part as text; and in spans
        got, stats = _sorted([mixed["sam"][0], mixed["bam"][1], mixed["sam"][2]], str(tmp_path / "mixed2.bam"), range_bytes=40_000)
        assert got == want and stats["retid_inputs"] == 1 and stats["ranges"] > 3
        got, stats = _sorted(mixed["sam"], str(tmp_path / "all_sam.bam"))
        assert got == want and stats["input"] == "sam"
        got, stats = _sorted([mixed["sam"][0], mixed["bam"][1], mixed["sam"][2]], str(tmp_path / "mixed_spans.bam"), range_bytes=40_000,
                             memory_bytes=(bam_stats["stream_bytes"] - 4) // 4)
        assert got == want and stats["spans"] >= 4


def test_a_name_in_no_dictionary_is_refused_with_its_line(mixed, tmp_path):
    from svision_amd import sort
    bare = str(tmp_path / "bare.sam")
    lines = _read(mixed["sam"][2]).split(b"\n")
    cols = lines[4].split(b"\t")
    cols[2] = b"chrNowhere"
    lines[4] = b"\t".join(cols)
    with open(bare, "wb") as f:
        f.write(b"\n".join(lines))
    with pytest.raises(sort.SortWriteError) as exc:
        sort.sort_bam([mixed["bam"][0], bare], str(tmp_path / "never.bam"), device=DEV)
    assert "bare.sam" in str(exc.value) and "line 5:" in str(exc.value), str(exc.value)
    assert sorted(os.listdir(str(tmp_path))) == ["bare.sam"]


# ---- 5. in spans ----
def test_different_dictionaries_in_spans(dictionaries, tmp_path):
    paths, one, one_records, _merged = dictionaries
    want, core_stats = _sorted(paths, str(tmp_path / "core.bam"))
    record_bytes = sum(len(r) for r in one_records)
    assert core_stats["stream_bytes"] == record_bytes + 4
    for tables in ("fixed", "dynamic"):
        core = want if tables == "fixed" else _sorted(paths, str(tmp_path / "core_dyn.bam"), tables=tables)[0]
        got, stats = _sorted(paths, str(tmp_path / "spans.bam"), tables=tables, memory_bytes=record_bytes // 5, range_bytes=1 << 15)
        assert got == core
        assert stats["spans"] > 1 and stats["span_range_reads"] >= stats["spans"] and stats["retid_inputs"] == 2 and stats["ranges"] > 6
        assert stats["stream_bytes"] < core_stats["stream_bytes"]
    assert _sorted(one, str(tmp_path / "one.bam"))[0] == want


# ---- 6. one input ----
def test_one_input_is_what_it_was(shuffled, tmp_path):
    _d, path, sorted_path, text, refs, records = shuffled
    a, a_stats = _sorted(path, str(tmp_path / "a.bam"))
    b, b_stats = _sorted([path], str(tmp_path / "b.bam"))
    same = lambda st: {k: v for k, v in st.items() if k not in ("seconds", "memory_bytes")}      # (the budget: half of what is free at the call)
    assert a == b and same(a_stats) == same(b_stats)
    assert a_stats["inputs"] == 1 and a_stats["retid_inputs"] == 0 and a_stats["seconds"]["retid"] == 0.0
    # the records of the file the stable sort of the test side wrote
    assert mc.raw_bam(str(tmp_path / "a.bam"))[2] == mc.raw_bam(sorted_path)[2]
    # an input without a record is one of several like any other
    empty = mc.write_raw_bam(str(tmp_path / "empty.in.bam"), text, refs, [])
    c, c_stats = _sorted([empty, path, empty], str(tmp_path / "c.bam"))
    assert c == a and c_stats["input_records"] == [0, len(records), 0] and c_stats["inputs"] == 3
    with open(str(tmp_path / "head.sam"), "w") as f:
        f.write(text)
    d, d_stats = _sorted([path, str(tmp_path / "head.sam")], str(tmp_path / "d.bam"))
    assert d == a and d_stats["input_records"] == [len(records), 0]


# ---- 7. refusals ----
def test_refusals_leave_nothing_behind(shuffled, tmp_path):
    from svision_amd import sort
    _d, path, _sorted_path, text, refs, records = shuffled
    src = str(tmp_path / "in")
    out_dir = str(tmp_path / "out")
    os.makedirs(src)
    os.makedirs(out_dir)
    good = mc.write_raw_bam(os.path.join(src, "good.bam"), text + "@RG\tID:rg\tSM:one\n", refs, records[:200])
    other_length = mc.write_raw_bam(os.path.join(src, "other_length.bam"), text, [refs[0], (refs[1][0], refs[1][1] + 1)], records[200:300])
    other_rg = mc.write_raw_bam(os.path.join(src, "other_rg.bam"), text + "@RG\tID:rg\tSM:two\n", refs, records[200:300])
    cut = os.path.join(src, "cut.bam")
    with open(cut, "wb") as f:
        f.write(_read(path)[:40_000])
    beyond = mc.write_raw_bam(os.path.join(src, "beyond.bam"), text, refs[::-1],
                              records[200:300] + [mc.with_refs(records[300], len(refs), -1)] + records[301:400])
    for second, words in ((other_length, ("good.bam", "other_length.bam", "chrB")), (other_rg, ("good.bam", "other_rg.bam", "RG:Z")),
                          (os.path.join(src, "missing.bam"), ("missing.bam",)), (cut, ("cut.bam",)), (beyond, ("beyond.bam",))):
        with pytest.raises(sort.SortWriteError) as exc:
            sort.sort_bam([good, second], os.path.join(out_dir, "never.bam"), device=DEV, range_bytes=1 << 15)
        assert all(w in str(exc.value) for w in words), str(exc.value)
        assert os.listdir(out_dir) == []
    with pytest.raises(ValueError):
        sort.sort_bam([], os.path.join(out_dir, "never.bam"), device=DEV)
    assert os.listdir(out_dir) == []


# ---- 8. the command lines (child processes: what the test is about) ----
@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from oracle import alexnet_ref
    from svision_amd.network import tf_checkpoint as ck
    prefix = str(tmp_path_factory.mktemp("ckpt") / "svision-cnn-model.ckpt")
    ck.write_checkpoint(prefix, alexnet_ref.random_params(seed=7))
    return prefix


def _env(extra):
    base = {k: v for k, v in os.environ.items() if k not in ("SVX_DEVICE_SORT", "SVX_BUILD_INDEX", "SVX_INGEST", "SVX_SORT_TABLES", "SVX_SORT_MEMORY")}
    return dict(base, PYTHONPATH=ROOT, **extra)


def test_module_command_line(dictionaries, tmp_path):
    paths, one, one_records, _merged = dictionaries
    want, _stats = _sorted(one, str(tmp_path / "one.bam"))
    out = str(tmp_path / "cli.bam")
    r = subprocess.run([sys.executable, "-m", "svision_amd.sort"] + paths + ["-o", out, "--device", DEV], capture_output=True, text=True, timeout=600,
                       env=_env({}), cwd=str(tmp_path))
    assert r.returncode == 0 and "%d records" % len(one_records) in r.stdout and "3 inputs" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert _pair(out) == want


def test_main_hands_one_input_on_as_a_str(tmp_path, monkeypatch):
    from svision_amd import sort
    calls = []

    def spy(*a, **kw):
        calls.append(a)
        kw["stats"].update(records=0, blocks=0, stored_blocks=0, dynamic_blocks=0, inflated_bytes=0, compressed_bytes=0, ranges=0, chunks=0, seconds={})
        return a[1]
    monkeypatch.setattr(sort, "sort_bam", spy)
    assert sort.main(["a.bam", "-o", "x.bam"]) == 0 and calls[-1] == ("a.bam", "x.bam")
    assert sort.main(["a.bam", "b.sam", "-o", "x.bam"]) == 0 and calls[-1] == (["a.bam", "b.sam"], "x.bam")


def test_svision_takes_a_list_under_the_switch(shuffled, checkpoint, tmp_path):
    """SVX_DEVICE_SORT=write ./SVision -b a,b,c: OUT/<a's stem>.merged.sorted.bam + .bai, then the VCF and segments/ of the run on the
    pre-sorted single file; without the switch the list is refused."""
    _d, _path, sorted_path, text, refs, records = shuffled
    third = len(records) // 3                                   # thirds of the shuffled file: ties keep the order the sorted file has
    parts = [mc.write_raw_bam(str(tmp_path / ("third%d.bam" % i)), text, refs, records[i * third:(i + 1) * third if i < 2 else None]) for i in range(3)]
    fasta = helpers.load_golden_fasta("collect_small.fa.gz")
    fa = str(tmp_path / "collect_small.fa")
    bam.write_fasta(fa, {n: fasta._seq[n] for n in fasta.references})
    args = ["-m", checkpoint, "-g", fa, "-n", "HGs", "-s", "3", "--window_size", "150000", "--batch_size", "64", "--debug", "-t", "1"]
    outs = {}
    for what, src, env in (("sorted", sorted_path, {}), ("list", ",".join(parts), {"SVX_DEVICE_SORT": "write"}), ("refused", ",".join(parts), {})):
        out = str(tmp_path / ("out_" + what))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "SVision"), "-o", out, "-b", src] + args, capture_output=True, text=True, timeout=900,
                           env=_env(dict(env, SVX_TIMING="1")))
        if what == "refused":
            said = r.stdout + r.stderr + "".join(_read(os.path.join(out, n)).decode("latin-1") for n in os.listdir(out) if os.path.isfile(os.path.join(out, n)))
            assert r.returncode != 0 and "python -m svision_amd.sort" in said, said[-3000:]
            assert not [n for n in os.listdir(out) if n.endswith((".bam", ".bai", ".vcf"))] and not os.path.exists(os.path.join(out, "segments"))
            continue
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        seg = os.path.join(out, "segments")
        outs[what] = (_read(os.path.join(out, "HGs.svision.s3.vcf")), {f: _read(os.path.join(seg, f)) for f in sorted(os.listdir(seg))})
    written = os.path.join(str(tmp_path / "out_list"), "third0.merged.sorted.bam")
    assert os.path.exists(written) and os.path.exists(written + ".bai")
    assert mc.raw_bam(written)[2] == mc.raw_bam(sorted_path)[2]
    assert outs["sorted"][0].count(b"\n") > 20 and outs["list"] == outs["sorted"]
