"""sort_bam(..., drop_tags= / keep_tags=) (svision_amd/sort.py, sort_sources._tags, svx_record_tags_measure / svx_record_tags_write): the
two files must be, byte for byte, those that sort_bam WITHOUT the switch writes for the same inputs whose records were filtered on the
host by tests/tagcases.py's walker and written by the same test-side writer.  Drop and keep; in one piece and in spans; dynamic tables;
a .csi; three inputs of which one is renumbered and one renamed under ``retag``; a BAM through a FIFO under either ``pipe_bam``; the
refusals; the default road; every range read once; and one SVX_DEVICE_SORT=write command line."""
import gzip
import os
import subprocess
import sys
import threading

import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from tests import baicases, helpers, mergecases as mc, retagcases as rc, sortcases, tagcases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 100                                                         # records an input
HD = "@HD\tVN:1.6\tSO:unsorted\n"
DROP = ("fi", "fp", "ri", "rp", "mv", "XD")
KEEP = ("RG", "NM", "MD", "SA")
FILTERS = {"drop": dict(drop_tags=list(DROP)), "keep": dict(keep_tags=",".join(KEEP))}
RANGE = 1 << 13                                               # compressed bytes a range: several ranges an input


def _pair(path, ext=".bai"):
    return open(path, "rb").read(), open(path + ext, "rb").read()


def _sorted(inputs, out, ext=".bai", **kw):
    from svision_amd import sort
    stats = {}
    assert sort.sort_bam(inputs, out, device=DEV, stats=stats, **kw) == out
    assert not [n for n in os.listdir(os.path.dirname(out)) if n.endswith(".tmp") or ".spool." in n]
    return _pair(out, ext), stats


def _tagged(records, rg=b"1"):
    """Every record with optional fields behind its own, in turn: the kinetics arrays of the read's length with kept fields between
    them, a base-modification pair, a move table, kept fields only, none, removed fields only, every type once; a few records
    carry a kinetics-sized B:S array of 20,000 elements."""
    out = []
    for i, r in enumerate(records):
        l_seq = int.from_bytes(r[20:24], "little")
        kin = lambda tag: rc.b_array(tag, "C", l_seq)
        kinds = (rc.fixed("NM", "i", i) + kin("fi") + kin("fp") + rc.z("RG", rg) + kin("ri") + kin("rp") + rc.z("MD", b"10A5^AC6"),
                 rc.z("MM", b"C+m,1,5,0;" * 30) + rc.b_array("ML", "C", 90) + rc.fixed("NM", "C", 3),
                 rc.b_array("mv", "c", 700 + i) + rc.z("RG", rg) + rc.z("SA", b"chrB,100,+,50M,60,0;"),
                 rc.z("RG", rg) + rc.fixed("NM", "s", 2) + rc.z("MD", b""), b"", tc.R1 + kin("fi"),
                 b"".join(tc.of_type(("XD", "NM", "q%d" % (k % 10))[k % 3], kind, k) for k, kind in enumerate(tc.TYPES)),
                 rc.z("RG", b"solo") + tc.R1 + rc.z("PG", b"aln"))
        fields = kinds[i % len(kinds)]
        if i % 41 == 7:
            fields = rc.fixed("NM", "i", 1) + rc.b_array("fi", "S", 20000) + fields
        out.append(rc.with_fields(r, fields))
    return out


def _filtered(records, mode):
    new = [tc.walk(r, mode, DROP if mode == "drop" else KEEP) for r in records]
    assert None not in new
    return new


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """One unsorted BAM of 3 N tagged records (the writer cuts its blocks every 0xFF00 bytes: records straddle them); the same records
    as three inputs whose @RG 1 collide, the 2nd with its dictionary turned round; per mode the filtered records and files and the
    oracle's two files for them (sort_bam without the switch), and the unfiltered run's files and statistics."""
    d = str(tmp_path_factory.mktemp("sort_tags"))
    path, _sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), d, 53)
    _text, refs, records = mc.raw_bam(path)
    records = _tagged(records[:3 * N])
    sq = mc.sq(refs)
    rg = ["@RG\tID:1\tSM:s\tPU:cell_%s\n" % c for c in "abc"]
    solo, pg = "@RG\tID:solo\tSM:s\n", "@PG\tID:aln\tPN:aln\n"
    heads = [HD + sq + rg[0] + solo + pg, HD + mc.sq(refs[::-1]) + rg[1], HD + sq + rg[2]]

    def write(tag, recs):
        one = mc.write_raw_bam(os.path.join(d, "one.%s.bam" % tag), HD + sq + rg[0] + solo + pg, refs, recs)
        parts = [mc.write_raw_bam(os.path.join(d, "part%d.%s.bam" % (k, tag)), heads[k], refs[::-1] if k == 1 else refs,
                                  [mc.renumbered(r, refs, refs[::-1]) for r in recs[k * N:(k + 1) * N]] if k == 1 else recs[k * N:(k + 1) * N])
                 for k in range(3)]
        return one, parts
    s = dict(dir=d, refs=refs, records=records, bytes=sum(len(r) for r in records))
    s["one"], s["parts"] = write("all", records)
    assert max(len(r) for r in records) > 0xFF00 // 2 and os.path.getsize(s["one"]) > 6 * RANGE
    s["plain"] = _sorted(s["one"], os.path.join(d, "plain.out.bam"), range_bytes=RANGE)
    for mode in ("drop", "keep"):
        new = _filtered(records, mode)
        one, parts = write(mode, new)
        s[mode] = dict(records=new, one=one, parts=parts, bytes=sum(len(r) for r in new), changed=sum(a != b for a, b in zip(records, new)),
                       want=_sorted(one, os.path.join(d, "want.%s.bam" % mode))[0])
        assert s[mode]["bytes"] < s["bytes"] * 3 // 4 and 0 < s[mode]["changed"] < 3 * N
    assert s["drop"]["records"] != s["keep"]["records"]
    return s


@pytest.mark.parametrize("mode", ["drop", "keep"])
def test_in_one_piece_the_files_of_the_filtered_input_every_range_read_once(sets, mode, tmp_path):
    from svision_amd import sort
    f = sets[mode]
    out = str(tmp_path / "out.bam")
    got, stats = _sorted(sets["one"], out, range_bytes=RANGE, **FILTERS[mode])
    assert got == f["want"]
    assert stats["tags_mode"] == mode and stats["tags_records"] == f["changed"] and stats["tags_bytes"] == sets["bytes"] - f["bytes"]
    assert stats["seconds"]["tags"] > 0 and set(stats["seconds"]) == set(sort.STAGES) and stats["spans"] == 1 and stats["records"] == 3 * N
    # the stream was allocated once by the ISIZE sum of the unfiltered file, and no range was read a second time
    plain = sets["plain"][1]
    assert stats["stream_bytes"] == plain["stream_bytes"] == sets["bytes"] + 4
    assert stats["ranges"] == plain["ranges"] >= 6 and stats["range_records"] == plain["range_records"]
    assert stats["range_reads"] == stats["ranges"] == plain["range_reads"] and stats["span_range_reads"] == 0
    # the output inflates with zlib, and its records are the filtered ones, every one of them
    stream = gzip.decompress(got[0])
    w = baicases.walk(out)
    assert w.stream == stream and len(w.offsets) == 3 * N
    _text, refs, records = mc.raw_bam(out)
    assert refs == sets["refs"] and sorted(records) == sorted(f["records"]) and all(tc.field_ends(r) is not None for r in records)
    seen = set(tc.tags_seen(records))
    assert (not seen & set(DROP)) if mode == "drop" else seen <= set(KEEP)


@pytest.mark.parametrize("mode", ["drop", "keep"])
def test_in_spans_and_ranges(sets, mode, tmp_path):
    f = sets[mode]
    got, stats = _sorted(sets["one"], str(tmp_path / "spans.bam"), memory_bytes=f["bytes"] // 4, range_bytes=RANGE, **FILTERS[mode])
    assert got == f["want"]
    assert stats["spans"] >= 3 and stats["ranges"] >= 6 and stats["span_range_reads"] >= stats["spans"] and stats["tags_records"] == f["changed"]
    assert stats["range_reads"] == stats["ranges"] + stats["span_range_reads"]
    # a budget between the filtered and the unfiltered size: the decision is the unfiltered size's -- spans, if one only
    got, stats = _sorted(sets["one"], str(tmp_path / "between.bam"), memory_bytes=(f["bytes"] + sets["bytes"]) // 2, **FILTERS[mode])
    assert got == f["want"] and stats["spans"] == 1 and stats["span_range_reads"] > 0


def test_dynamic_tables_and_a_csi(sets, tmp_path):
    for mode, kw, ext in (("drop", dict(tables="dynamic"), ".bai"), ("keep", dict(index_format="csi"), ".csi"), ("drop", dict(tables="dynamic", index_format="csi"), ".csi")):
        want = _sorted(sets[mode]["one"], str(tmp_path / "want.bam"), ext, **kw)[0]
        got, stats = _sorted(sets["one"], str(tmp_path / "got.bam"), ext, **kw, **FILTERS[mode])
        assert got == want and stats["tags_mode"] == mode
        assert (stats["dynamic_blocks"] > 0) == ("tables" in kw) and got[0] != sets["plain"][0][0]


@pytest.mark.parametrize("mode", ["drop", "keep"])
def test_three_inputs_one_renumbered_one_renamed(sets, mode, tmp_path):
    """Input 2 has its dictionary turned round (svx_record_retid) and the @RG 1 of inputs 2 and 3 collide with input 1's: under
    ``retag`` their records' RG:Z values are rewritten, then filtered -- retag first."""
    f = sets[mode]
    want, want_stats = _sorted(f["parts"], str(tmp_path / "want.bam"), retag=True)
    got, stats = _sorted(sets["parts"], str(tmp_path / "got.bam"), retag=True, range_bytes=RANGE, **FILTERS[mode])
    assert got == want
    assert stats["inputs"] == 3 and stats["retid_inputs"] == 1 and stats["retag_inputs"] == 2 and stats["retag_records"] == want_stats["retag_records"] > 0
    assert stats["tags_records"] == f["changed"] and stats["tags_bytes"] == sets["bytes"] - f["bytes"]
    assert stats["ranges"] < stats["range_reads"] <= 2 * stats["ranges"]     # (a run that also retags takes retag's road: a second read)
    got, stats = _sorted(sets["parts"], str(tmp_path / "spans.bam"), retag=True, memory_bytes=f["bytes"] // 4, range_bytes=RANGE, **FILTERS[mode])
    assert got == want and stats["spans"] >= 3 and stats["tags_records"] == f["changed"]
    # without retag the three inputs' records under the first input's read groups would be refused; two of them under one @RG line are not
    want = _sorted([f["parts"][0], f["parts"][0]], str(tmp_path / "twice.want.bam"))[0]
    got, stats = _sorted([sets["parts"][0], sets["parts"][0]], str(tmp_path / "twice.bam"), **FILTERS[mode])
    assert got == want and stats["range_reads"] == stats["ranges"] and stats["retag_inputs"] == 0


class Fifo:
    """A FIFO in ``d`` that a daemon thread writes ``data`` into (BrokenPipeError ignored: the reader may close early)."""

    def __init__(self, d, data, name="fifo"):
        self.path = os.path.join(str(d), name)
        os.mkfifo(self.path)

        def feed():
            try:
                with open(self.path, "wb") as f:
                    f.write(data)
            except BrokenPipeError:
                pass
        self.thread = threading.Thread(target=feed, daemon=True)
        self.thread.start()

    def done(self):
        self.thread.join(30)
        ended = not self.thread.is_alive()
        os.unlink(self.path)
        return ended


@pytest.mark.parametrize("pipe_bam", ["spool", "stream"])
def test_a_bam_through_a_fifo_is_sorted_from_its_copy(sets, pipe_bam, tmp_path):
    data = open(sets["one"], "rb").read()
    for mode in ("drop", "keep"):
        fifo = Fifo(tmp_path, data, "fifo." + mode)
        got, stats = _sorted(fifo.path, str(tmp_path / ("out.%s.bam" % mode)), pipe_bam=pipe_bam, **FILTERS[mode])
        assert fifo.done()
        assert got == sets[mode]["want"]
        assert stats["pipe"]["mode"] == "bam_spooled" and stats["pipe"]["holds"] == "bam" and stats["tags_records"] == sets[mode]["changed"]
    # without the switch "stream" takes the pipe in one pass, as ever
    fifo = Fifo(tmp_path, data, "fifo.plain")
    got, stats = _sorted(fifo.path, str(tmp_path / "plain.bam"), pipe_bam=pipe_bam)
    assert fifo.done() and got == sets["plain"][0] and (stats["pipe"]["mode"] == "bam_spooled") == (pipe_bam == "spool")


def test_refusals_leave_nothing_behind(sets, tmp_path):
    from svision_amd import sort
    src, out_dir = str(tmp_path / "in"), str(tmp_path / "out")
    os.makedirs(src)
    os.makedirs(out_dir)
    never = os.path.join(out_dir, "never.bam")
    text = os.path.join(src, "text.sam")
    with open(text, "w") as f:
        f.write(HD + mc.sq(sets["refs"]) + "t0\t0\t%s\t6\t9\t8M\t*\t0\t0\tACGTACGT\t*\tfi:B:C,1,2\n" % sets["refs"][0][0])
    for inputs, kw, switch in ((text, FILTERS["drop"], "--drop-tags"), ([sets["one"], text], FILTERS["keep"], "--keep-tags")):
        with pytest.raises(sort.SortWriteError) as exc:
            sort.sort_bam(inputs, never, device=DEV, **kw)
        assert "text.sam" in str(exc.value) and switch in str(exc.value) and "BAM" in str(exc.value), str(exc.value)
        assert os.listdir(out_dir) == []
    fifo = Fifo(src, open(text, "rb").read())                   # the same text on a pipe
    with pytest.raises(sort.SortWriteError, match="--drop-tags"):
        sort.sort_bam(fifo.path, never, device=DEV, **FILTERS["drop"])
    assert fifo.done() and os.listdir(out_dir) == []
    # a record whose optional fields are malformed: an unknown type, in the middle of the file
    records = list(sets["records"][:N])
    records[N // 2] = rc.with_fields(records[N // 2], b"XXQv\0")
    bad = mc.write_raw_bam(os.path.join(src, "bad.bam"), HD + mc.sq(sets["refs"]), sets["refs"], records)
    for kw in (FILTERS["drop"], dict(FILTERS["keep"], memory_bytes=1 << 18)):
        with pytest.raises(sort.SortWriteError) as exc:
            sort.sort_bam(bad, never, device=DEV, range_bytes=RANGE, **kw)
        assert "bad.bam" in str(exc.value) and "malformed" in str(exc.value), str(exc.value)
        assert os.listdir(out_dir) == []
    _sorted(bad, os.path.join(out_dir, "unfiltered.bam"))       # without the switch nobody walks the fields: sorted as ever
    # bad lists: a ValueError before anything is opened
    for kw in (dict(drop_tags="CG"), dict(drop_tags="fi", keep_tags="RG"), dict(keep_tags=["R"]), dict(drop_tags="fi,fi")):
        with pytest.raises(ValueError):
            sort.sort_bam("/nonexistent.bam", never, device=DEV, **kw)


def test_the_default_road_is_the_run_it_was(sets, tmp_path, monkeypatch):
    monkeypatch.delenv("SVX_SORT_DROP_TAGS", raising=False)
    monkeypatch.delenv("SVX_SORT_KEEP_TAGS", raising=False)
    never, never_stats = sets["plain"]
    got, stats = _sorted(sets["one"], str(tmp_path / "none.bam"), range_bytes=RANGE, drop_tags=None, keep_tags=None)
    assert got == never
    for st in (stats, never_stats):
        assert st["tags_mode"] is None and st["tags_records"] == 0 and st["tags_bytes"] == 0 and st["seconds"]["tags"] == 0.0
    same = lambda st: {k: v for k, v in st.items() if k not in ("seconds", "memory_bytes")}
    assert same(stats) == same(never_stats)
    got, stats = _sorted(sets["one"], str(tmp_path / "empty.bam"), range_bytes=RANGE, drop_tags=())        # an empty drop list: off
    assert got == never and stats["tags_mode"] is None and stats["seconds"]["tags"] == 0.0
    # the environment turns it on where the arguments say nothing
    monkeypatch.setenv("SVX_SORT_DROP_TAGS", ",".join(DROP))
    got, stats = _sorted(sets["one"], str(tmp_path / "env.bam"))
    assert got == sets["drop"]["want"] and stats["tags_mode"] == "drop"
    monkeypatch.delenv("SVX_SORT_DROP_TAGS")
    monkeypatch.setenv("SVX_SORT_KEEP_TAGS", ",".join(KEEP))
    assert _sorted(sets["one"], str(tmp_path / "env_keep.bam"))[0] == sets["keep"]["want"]


def test_the_module_command_line(sets, tmp_path):
    """``python -m svision_amd.sort --drop-tags``: the oracle's files and the summary line; a bad environment value is an argument error."""
    out = str(tmp_path / "cli.bam")
    env = {k: v for k, v in os.environ.items() if k not in ("SVX_SORT_DROP_TAGS", "SVX_SORT_KEEP_TAGS")}
    r = subprocess.run([sys.executable, "-m", "svision_amd.sort", sets["one"], "-o", out, "--drop-tags", ",".join(DROP)], capture_output=True, text=True,
                       timeout=600, env=dict(env, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    f = sets["drop"]
    assert _pair(out) == f["want"]
    assert "--drop-tags): %d record(s) changed, %d bytes removed" % (f["changed"], sets["bytes"] - f["bytes"]) in r.stdout, r.stdout
    r = subprocess.run([sys.executable, "-m", "svision_amd.sort", sets["one"], "-o", out], capture_output=True, text=True, timeout=600,
                       env=dict(env, PYTHONPATH=ROOT, SVX_SORT_KEEP_TAGS="RG,R"))
    assert r.returncode == 2 and "SVX_SORT_KEEP_TAGS" in r.stderr


# ---- SVX_DEVICE_SORT=write ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from oracle import alexnet_ref
    from svision_amd.network import tf_checkpoint as ck
    prefix = str(tmp_path_factory.mktemp("ckpt") / "svision-cnn-model.ckpt")
    ck.write_checkpoint(prefix, alexnet_ref.random_params(seed=7))
    return prefix


def _cli(args, env):
    base = {k: v for k, v in os.environ.items() if k not in ("SVX_DEVICE_SORT", "SVX_BUILD_INDEX", "SVX_INGEST", "SVX_SORT_DROP_TAGS", "SVX_SORT_KEEP_TAGS")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "SVision")] + list(args), capture_output=True, text=True, timeout=900,
                          env=dict(base, PYTHONPATH=ROOT, SVX_TIMING="1", **env))


def test_device_sort_write_inherits_the_environment(checkpoint, tmp_path):
    """SVX_DEVICE_SORT=write with SVX_SORT_DROP_TAGS set: the VCF of the run without it -- the caller reads no optional field -- and a
    smaller sorted file, which holds none of the dropped fields."""
    from svision_amd.io import bam
    path, _sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), tmp_path, 21)
    text, refs, records = mc.raw_bam(path)
    tagged = mc.write_raw_bam(str(tmp_path / "tagged.bam"), text, refs,
                              [rc.with_fields(r, rc.fixed("NM", "i", 1) + rc.b_array("fi", "C", int.from_bytes(r[20:24], "little")) + rc.z("RG", b"1")) for r in records])
    fasta = helpers.load_golden_fasta("collect_small.fa.gz")
    fa = str(tmp_path / "collect_small.fa")
    bam.write_fasta(fa, {n: fasta._seq[n] for n in fasta.references})
    args = ["-m", checkpoint, "-g", fa, "-n", "HGs", "-s", "3", "--window_size", "150000", "--batch_size", "64", "--debug", "-t", "1"]
    vcf, size = {}, {}
    for what, env in (("plain", {}), ("drop", {"SVX_SORT_DROP_TAGS": "fi,fp,ri,rp"})):
        out = str(tmp_path / ("out_" + what))
        r = _cli(["-o", out, "-b", tagged] + args, dict(env, SVX_DEVICE_SORT="write"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        written = os.path.join(out, "tagged.sorted.bam")
        assert os.path.exists(written + ".bai")
        vcf[what], size[what] = open(os.path.join(out, "HGs.svision.s3.vcf"), "rb").read(), os.path.getsize(written)
        seen = set(tc.tags_seen(mc.raw_bam(written)[2]))
        assert seen == ({"NM", "RG"} if what == "drop" else {"NM", "fi", "RG"})
    assert vcf["drop"] == vcf["plain"] and vcf["plain"].count(b"\n") > 20 and size["drop"] < size["plain"]
