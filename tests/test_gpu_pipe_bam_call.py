"""A sample straight from a BAM on a pipe (svision_amd/ingest_sort.py under ``pipe_bam="stream"`` / SVX_PIPE_BAM=stream): load_sample on a
FIFO against load_sample on the same bytes as a file -- every table array, the name list, the bases, the scan --, on the cases of
tests/pipebam_cases.py at ranges that cut records, grow and hold the whole stream; the pipe among several inputs; the failures, in the
file road's words, that end the writer and leave nothing; and the command line against its run on the sorted, indexed file."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from svision_amd.io import bam
from tests import helpers, htslike, pipebam_cases as pb, samtext, sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_SV = 50
RANGES = (64 << 10, 256 << 10, None)
NO_FASTA = bam.Fasta(sequences={"chrA": b"ACGT"})


def _load(src, with_seq=True, range_bytes=None, stats=None, **kw):
    from svision_amd import ingest_sort
    return ingest_sort.load_sample(src, NO_FASTA, MIN_SV, device=DEV, with_seq=with_seq, range_bytes=range_bytes, stats=stats, **kw)


def _same(got, want, with_seq=True, what=""):
    sortcases.assert_same_table(got.table, want.table, with_seq=with_seq, what=what)
    assert (got.table.seq_packed is None) == (not with_seq)
    assert np.array_equal(got.gap_off, want.gap_off) and np.array_equal(got.stats, want.stats), what
    assert got.gaps.dtype == want.gaps.dtype and got.gaps.tobytes() == want.gaps.tobytes(), what
    assert np.array_equal(got.table.ref_span, want.table.ref_span), what


@pytest.fixture(scope="module")
def want():
    """name -> (load_sample(the file) with bases, without): loaded once, left unchanged."""
    return {name: (_load(pb.case(name)["path"], True), _load(pb.case(name)["path"], False)) for name in pb.NAMES if name != "none"}


@pytest.mark.parametrize("range_bytes", RANGES, ids=["64K", "256K", "default"])
@pytest.mark.parametrize("name", [n for n in pb.NAMES if n != "none"])
def test_the_pipe_gives_the_sample_of_the_file(want, name, range_bytes, tmp_path):
    c = pb.case(name)
    for with_seq in (True, False):
        fifo, stats = pb.Fifo(tmp_path, c["data"]), {}
        got = _load(fifo.path, with_seq, range_bytes, stats, pipe_bam="stream")
        assert fifo.done() and not fifo.broke
        _same(got, want[name][0 if with_seq else 1], with_seq, (name, range_bytes, with_seq))
        assert stats["inputs"] == ["bam_pipe"] and stats["records"] == c["n"] and stats["host_lines"] == 0
        assert stats["pipes"][0]["bytes"] == len(c["data"]) and stats["seconds"]["pack"] == 0
        assert os.listdir(str(tmp_path)) == []
    if name == "ont" and range_bytes == 64 << 10:
        assert stats["ranges"] <= c["n"] + 1                    # no range without a record is handed on: each grew until one completed


def test_a_header_and_no_record(tmp_path):
    from svision_amd import ingest_sort
    fifo = pb.Fifo(tmp_path, pb.case("none")["data"])
    with pytest.raises(ingest_sort.SortIngestError, match="holds no record"):
        _load(fifo.path, pipe_bam="stream")
    assert fifo.done() and os.listdir(str(tmp_path)) == []


def test_the_switch(tmp_path, monkeypatch):
    """Off by default and under "spool" / "0": the refusal of before, which now names the switch; the environment turns it on."""
    from svision_amd import ingest_sort
    c = pb.case("one")
    monkeypatch.delenv("SVX_PIPE_BAM", raising=False)
    for kw in ({}, {"pipe_bam": "spool"}, {"pipe_bam": "0"}):
        fifo = pb.Fifo(tmp_path, c["data"])
        with pytest.raises(ingest_sort.SortIngestError, match="SVX_DEVICE_SORT=write") as exc:
            _load(fifo.path, **kw)
        assert "a BAM on a pipe is not taken" in str(exc.value) and "SVX_PIPE_BAM=stream" in str(exc.value) and "\n" not in str(exc.value)
        assert fifo.done() and os.listdir(str(tmp_path)) == []
    with pytest.raises(ingest_sort.SortIngestError, match="SVX_PIPE_BAM"):
        _load(c["path"], pipe_bam="sideways")
    monkeypatch.setenv("SVX_PIPE_BAM", "stream")
    fifo, stats = pb.Fifo(tmp_path, c["data"]), {}
    assert len(_load(fifo.path, stats=stats).table) == 1 and stats["inputs"] == ["bam_pipe"] and fifo.done()


def test_the_pipe_among_several_inputs(tmp_path):
    """[a.bam, fifo(b.bam), c.sam] == [a.bam, b.bam, c.sam]: the parts' dictionaries differ, so b's records are renumbered, and every
    part has records at the same (reference, position): ties come out in list order, then stream order."""
    c = pb.case("flush")
    recs = c["recs"][:90]
    refs = {"a": [("chr0", 50_000)] + pb.REFS, "b": pb.REFS[::-1] + [("chrZ", 70_000)], "c": pb.REFS}
    paths = {}
    for k in "abc":
        names = [r for r, _n in refs[k]]
        mine = [dict(r, qname="%s_%s" % (r["qname"], k), tid=names.index(pb.REFS[r["tid"]][0]), tags=[("NM", "i", 300 + i)]) for i, r in enumerate(recs)]
        paths[k] = str(tmp_path / (k + (".sam" if k == "c" else ".bam")))
        if k == "c":
            with open(paths[k], "wb") as f:
                f.write(samtext.text(refs[k], mine, header=samtext.header_text(refs[k])))
        else:
            htslike.write_bam(paths[k], refs[k], [samtext.for_htslike(r) for r in mine], level=1, policy="stream", header_text=samtext.header_text(refs[k]), index=False)
    want = _load([paths["a"], paths["b"], paths["c"]])
    data = open(paths["b"], "rb").read()
    for range_bytes in (64 << 10, None):
        fifo, stats = pb.Fifo(tmp_path, data), {}
        got = _load([paths["a"], fifo.path, paths["c"]], range_bytes=range_bytes, stats=stats, pipe_bam="stream")
        assert fifo.done() and not fifo.broke
        _same(got, want, True, range_bytes)
        assert stats["inputs"] == ["bam", "bam_pipe", "sam"] and stats["records"] == 270
    table = got.table
    where = {}
    for i, nid in enumerate(table.name_id):                     # every read's three copies have one key: part a, b, c in that order
        stem, k = table.names[int(nid)].rsplit("_", 1)
        where.setdefault(stem, {})[k] = i
    assert len(where) == 90 and all(w["a"] < w["b"] < w["c"] for w in where.values())
    assert table.references == ["chr0", "chrA", "chrB", "chrZ"]


def _third_range(data, range_bytes):
    """The stream offset of the first member that starts behind two chunks of ``range_bytes`` -- in the third range --, and its length."""
    spans = pb.members(data)
    return next((at, n) for at, n in spans if at > 2 * range_bytes + 4096)


def test_failures_say_what_the_file_road_says_and_end_the_writer(tmp_path):
    from svision_amd import ingest_sort
    c = pb.case("hifi")
    range_bytes = 256 << 10                                     # (the third range lies behind what the file road's header reader inflates)
    at, n = _third_range(c["data"], range_bytes)
    flipped = bytearray(c["data"])
    flipped[at + n // 2] ^= 0x55
    cut = pb.members(c["data"])[len(pb.members(c["data"])) // 3][0]
    for what, data in (("flipped", bytes(flipped)), ("cut", c["data"][:cut] + htslike.EOF_BLOCK)):
        path = str(tmp_path / (what + ".bam"))
        with open(path, "wb") as f:
            f.write(data)
        with pytest.raises(ingest_sort.SortIngestError) as of_file:
            _load(path, range_bytes=range_bytes)
        before = sorted(os.listdir(str(tmp_path)))
        fifo = pb.Fifo(tmp_path, data)
        with pytest.raises(ingest_sort.SortIngestError) as of_pipe:
            _load(fifo.path, range_bytes=range_bytes, pipe_bam="stream")
        assert fifo.done() and (fifo.broke or what == "cut")   # (the cut stream is short: it may be written whole before the failure)
        assert sorted(os.listdir(str(tmp_path))) == before
        said, want = str(of_pipe.value), str(of_file.value).replace(path, fifo.path).replace("file offset", "stream offset")
        assert said == want and "\n" not in said, (said, want)
        assert ("offset %d" % at in said and ("CRC32" in said or "corrupt" in said)) if what == "flipped" else "is cut inside a record" in said


# ---- the command line (a child process with the BAM on standard input: what the test is about) ----
@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from oracle import alexnet_ref
    from svision_amd.network import tf_checkpoint as ck
    prefix = str(tmp_path_factory.mktemp("ckpt") / "svision-cnn-model.ckpt")
    ck.write_checkpoint(prefix, alexnet_ref.random_params(seed=7))
    return prefix


def _env(extra):
    base = {k: v for k, v in os.environ.items() if k not in ("SVX_DEVICE_SORT", "SVX_BUILD_INDEX", "SVX_INGEST", "SVX_SORT_TABLES", "SVX_SORT_MEMORY",
                                                             "SVX_PIPE_BAM")}
    return dict(base, PYTHONPATH=ROOT, **extra)


def test_svision_calls_from_a_bam_on_standard_input(checkpoint, tmp_path):
    """SVX_PIPE_BAM=stream SVX_DEVICE_SORT=1 ./SVision -b - fed an unsorted BAM: the VCF and segments/ of the run on the same records as a
    sorted, indexed file; no alignment file appears in OUT/.  Without SVX_PIPE_BAM the run is refused in one line that names it.  The
    BAM is the golden set's, shuffled, as in the other command-line tests: the simulated hifi case (2.5-fold) yields no call to compare."""
    path, sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), tmp_path, 21)
    c = dict(data=open(path, "rb").read())
    fasta = helpers.load_golden_fasta("collect_small.fa.gz")
    fa = str(tmp_path / "collect_small.fa")
    bam.write_fasta(fa, {n: fasta._seq[n] for n in fasta.references})
    args = ["-m", checkpoint, "-g", fa, "-n", "HGs", "-s", "3", "--window_size", "150000", "--batch_size", "64", "--debug", "-t", "1"]
    outs = {}
    for what, src, env in (("file", sorted_path, {}), ("stdin", "-", {"SVX_DEVICE_SORT": "1", "SVX_PIPE_BAM": "stream"}), ("refused", "-", {"SVX_DEVICE_SORT": "1"})):
        out = str(tmp_path / ("out_" + what))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "SVision"), "-o", out, "-b", src] + args, input=c["data"] if src == "-" else None,
                           capture_output=True, timeout=900, env=_env(dict(env, SVX_TIMING="1")))
        stdout, stderr = r.stdout.decode(), r.stderr.decode()
        if what == "refused":
            logs = [os.path.join(out, f) for f in os.listdir(out) if f.startswith("SVision_") and f.endswith(".log")]
            said = [l for f in logs for l in open(f).read().splitlines() if "[ERROR" in l]         # (the run's errors go to its log file)
            assert r.returncode != 0 and len(said) == 1 and "SVX_PIPE_BAM=stream" in said[0], "\n".join(said) + stdout[-2000:] + stderr[-3000:]
            continue
        assert r.returncode == 0, (what, stdout[-2000:] + stderr[-3000:])
        seg = os.path.join(out, "segments")
        logs = [open(os.path.join(out, f)).read()[-3000:] for f in os.listdir(out) if f.endswith(".log")]
        assert os.path.exists(os.path.join(out, "HGs.svision.s3.vcf")), (what, sorted(os.listdir(out)), stdout[-2000:] + stderr[-2000:], logs)
        outs[what] = (open(os.path.join(out, "HGs.svision.s3.vcf"), "rb").read(), {f: open(os.path.join(seg, f), "rb").read() for f in sorted(os.listdir(seg))})
    assert not [f for _dir, _sub, names in os.walk(str(tmp_path / "out_stdin")) for f in names if f.endswith((".bam", ".bai")) or ".spool." in f]
    assert outs["file"][0].count(b"\n") > 20 and outs["file"][1] and outs["stdin"] == outs["file"]
