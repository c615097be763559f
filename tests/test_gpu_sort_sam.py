"""sort_bam on SAM text (svision_amd/sort.py over svx_sam.hip): three record sets -- the cases of tests/sam_cases.py, a shuffled
HiFi-shaped and an ONT-shaped set of svision_amd.synth -- each written twice, as SAM text and as an unsorted BAM of tests/htslike.py
under the same header text.  Both inputs must give the same two files, byte for byte: with fixed and dynamic tables, in one piece and
in spans, whatever the chunks of text.  The readers read the output, a text that changes between the passes is refused, and the
command lines take SAM text where SVX_DEVICE_SORT=write lets them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from svision_amd.io import bam
from tests import helpers, htslike, sam_cases, samtext, sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _synth_records(ont, seed):
    from svision_amd import synth
    cfg = synth.SimConfig(contigs=[("chrA", 900_000), ("chrB", 600_000)], coverage=2.5, seed=seed)
    if ont:
        cfg.lognormal, cfg.read_len_mean, cfg.err_rate, cfg.coverage = True, 12_000.0, 0.06, 2.0
    table, _genome, _svs = synth.simulate(cfg, with_seq=True)
    rng = np.random.default_rng(seed)
    recs = samtext.records_of_table(table, rng, tags=True)
    refs = list(zip(table.references, table.lengths))
    return refs, [recs[i] for i in rng.permutation(len(recs))]


def _write_pair(d, name, refs, recs):
    text = samtext.header_text(refs)
    sam_path, bam_path = os.path.join(d, name + ".sam"), os.path.join(d, name + ".unsorted.bam")
    with open(sam_path, "wb") as f:
        f.write(samtext.text(refs, recs, header=text, last_newline=name != "ont"))
    htslike.write_bam(bam_path, refs, [samtext.for_htslike(r) for r in recs], level=1, policy="stream", header_text=text, index=False)
    return sam_path, bam_path


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """name -> dict(sam, bam: the two inputs; n: records; host_lines: the lines the kernels leave to the host; out: sort_bam(bam)'s
    files per tables as bytes): written and sorted once."""
    from svision_amd import sort
    d = str(tmp_path_factory.mktemp("sort_sam"))
    out = {}
    for name, (refs, recs), host_lines in (("cases", (sam_cases.REFS, sam_cases.records()), len(sam_cases.refused_lines())),
                                           ("hifi", _synth_records(False, 5), 0), ("ont", _synth_records(True, 6), 0)):
        sam_path, bam_path = _write_pair(d, name, refs, recs)
        s = out[name] = dict(sam=sam_path, bam=bam_path, n=len(recs), host_lines=host_lines, dir=d, want={})
        for tables in ("fixed", "dynamic"):
            p = os.path.join(d, "%s.%s.from_bam.bam" % (name, tables))
            stats = {}
            sort.sort_bam(bam_path, p, device=DEV, tables=tables, stats=stats)
            assert "input" not in stats and "host_lines" not in stats
            s["want"][tables] = (open(p, "rb").read(), open(p + ".bai", "rb").read())
            s["room"] = stats["stream_bytes"] - 4
    assert out["hifi"]["n"] > 150 and out["ont"]["n"] > 100
    return out


def _same_files(s, tables, path):
    assert open(path, "rb").read() == s["want"][tables][0]
    assert open(path + ".bai", "rb").read() == s["want"][tables][1]
    assert not [n for n in os.listdir(os.path.dirname(path)) if n.endswith(".tmp")]


@pytest.mark.parametrize("tables", ["fixed", "dynamic"])
@pytest.mark.parametrize("name", ["cases", "hifi", "ont"])
def test_sam_and_bam_give_the_same_files(sets, name, tables, tmp_path):
    from svision_amd import sort
    s = sets[name]
    # the default chunk (one), and chunks smaller than the longest line: a boundary falls before, at and behind newlines
    for what, kw in (("default", {}), ("small", dict(range_bytes=30_011, chunk_bytes=3 * htslike.BLOCK))):
        out, stats = str(tmp_path / (what + ".bam")), {}
        assert sort.sort_bam(s["sam"], out, device=DEV, tables=tables, stats=stats, **kw) == out
        _same_files(s, tables, out)
        assert stats["input"] == "sam" and stats["host_lines"] == s["host_lines"] and stats["records"] == s["n"] and stats["spans"] == 1
        assert set(stats["seconds"]) == set(sort.STAGES) and stats["stream_bytes"] == s["room"] + 4
        assert (stats["ranges"] == 1) if what == "default" else (stats["ranges"] > 4), stats["ranges"]


@pytest.mark.parametrize("name", ["cases", "hifi", "ont"])
def test_in_spans(sets, name, tmp_path):
    from svision_amd import sort
    s = sets[name]
    budget = s["room"] // 5
    out, stats = str(tmp_path / "spans.bam"), {}
    sort.sort_bam(s["sam"], out, device=DEV, memory_bytes=budget, range_bytes=100_003, stats=stats)
    _same_files(s, "fixed", out)
    longest = max(len(r) for r in bam_records(s["want"]["fixed"][0]))
    assert stats["spans"] >= 5 and stats["span_range_reads"] >= stats["spans"] and stats["host_lines"] == s["host_lines"]
    assert stats["stream_bytes"] <= budget + 2 * longest + 4, (stats["stream_bytes"], budget, longest)


def bam_records(raw):
    """A BAM file's bytes -> its records' bytes."""
    import gzip
    import struct
    stream = gzip.decompress(raw)
    at = 8 + struct.unpack_from("<i", stream, 4)[0]
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    out = []
    while at < len(stream):
        n = 4 + struct.unpack_from("<i", stream, at)[0]
        out.append(stream[at:at + n])
        at += n
    return out


def test_the_readers_accept_it(sets, tmp_path):
    """The host reader and the device decoder on the file written from SAM text: the records of the text, in sortcases.order."""
    from svision_amd import ingest_gpu, sort
    s = sets["hifi"]
    out = str(tmp_path / "hifi.bam")
    sort.sort_bam(s["sam"], out, device=DEV)
    whole = bam.read_bam(out)
    head = bam.read_bam_header(out)
    assert whole.sort_order == "coordinate" and len(whole) == s["n"] and head.references == ["chrA", "chrB"]
    assert np.array_equal(sortcases.order(whole.tid, whole.pos, len(head.references)), np.arange(len(whole)))
    tids = list(range(len(head.references)))
    dec = ingest_gpu.DeviceDecoder(out, out + ".bai", head.references, head.lengths, head.header_text, DEV, threads=3)
    assert dec.usable(tids)
    seen = 0
    for finish, _arrays in dec.parts_pipelined(tids):
        tb = finish()
        t = int(tb.tid[0])
        host = whole.subset(np.flatnonzero(whole.tid == t))
        for fld in ("tid", "pos", "flag", "mapq", "l_seq"):
            assert np.array_equal(getattr(tb, fld), getattr(host, fld)), (t, fld)
        seen += len(host)
    assert seen == int((whole.tid >= 0).sum())


@pytest.mark.parametrize("spanned", [False, True], ids=["one_piece", "spans"])
@pytest.mark.parametrize("change", ["a_base_less", "a_line_less"])
def test_a_text_that_changes_between_the_passes(sets, tmp_path, monkeypatch, spanned, change):
    from svision_amd import sort
    s = sets["cases"]
    path = str(tmp_path / "changing.sam")
    raw = open(s["sam"], "rb").read()
    with open(path, "wb") as f:
        f.write(raw)
    lines = raw.split(b"\n")
    k = next(i for i, l in enumerate(lines) if l.startswith(b"seq_17\t"))
    if change == "a_line_less":
        del lines[k]
    else:
        cols = lines[k].split(b"\t")
        cols[9], cols[10] = cols[9][:-1], cols[10][:-1]
        lines[k] = b"\t".join(cols)
    changed = b"\n".join(lines)
    owner, step = (sort, "_pieces_spanned") if spanned else (sort.SamSource, "fill")
    real = getattr(owner, step)

    def rewrite_then(*a, **kw):
        with open(path, "wb") as f:
            f.write(changed)
        return real(*a, **kw)
    monkeypatch.setattr(owner, step, rewrite_then)
    before = sorted(os.listdir(str(tmp_path)))
    with pytest.raises(sort.SortWriteError, match="changed while it was sorted"):
        sort.sort_bam(path, str(tmp_path / "never.bam"), device=DEV, memory_bytes=s["room"] // 4 if spanned else None, range_bytes=50_000)
    assert sorted(os.listdir(str(tmp_path))) == before


@pytest.mark.parametrize("case", sam_cases.errors(), ids=[e[0] for e in sam_cases.errors()])
def test_errors_name_the_line_and_leave_nothing(tmp_path, case):
    from svision_amd import sort
    name, text, line_no, _code = case
    path = str(tmp_path / (name + ".sam"))
    with open(path, "wb") as f:
        f.write(text)
    before = sorted(os.listdir(str(tmp_path)))
    with pytest.raises(sort.SortWriteError) as exc:
        sort.sort_bam(path, str(tmp_path / "never.bam"), device=DEV, range_bytes=1 << 12)
    assert ("line %d:" % line_no if line_no else "@SQ") in str(exc.value), str(exc.value)
    assert sorted(os.listdir(str(tmp_path))) == before


def test_header_and_no_record_and_compressed_text(sets, tmp_path):
    import gzip
    from svision_amd import sort
    refs = sam_cases.REFS[:3]
    text = samtext.header_text(refs)
    sam_path, bam_path = str(tmp_path / "empty.sam"), str(tmp_path / "empty.in.bam")
    with open(sam_path, "wb") as f:
        f.write(text.encode())
    htslike.write_bam(bam_path, refs, [], level=1, policy="stream", header_text=text, index=False)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    stats = {}
    sort.sort_bam(sam_path, a, device=DEV, stats=stats)
    sort.sort_bam(bam_path, b, device=DEV)
    assert open(a, "rb").read() == open(b, "rb").read() and open(a + ".bai", "rb").read() == open(b + ".bai", "rb").read()
    assert stats["records"] == 0 and stats["input"] == "sam"
    gz = str(tmp_path / "text.sam.gz")
    with open(gz, "wb") as f:
        f.write(gzip.compress(open(sets["hifi"]["sam"], "rb").read(1 << 16)))
    with pytest.raises(sort.SortWriteError, match="compressed SAM is not taken"):
        sort.sort_bam(gz, str(tmp_path / "never.bam"), device=DEV)
    assert not os.path.exists(str(tmp_path / "never.bam"))


# ---- the command lines (child processes: what the test is about) ----
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


def test_module_command_line(sets, tmp_path):
    s = sets["hifi"]
    out = str(tmp_path / "cli.bam")
    r = subprocess.run([sys.executable, "-m", "svision_amd.sort", s["sam"], "-o", out], capture_output=True, text=True, timeout=600, env=_env({}),
                       cwd=str(tmp_path))
    assert r.returncode == 0 and "%d records" % s["n"] in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    _same_files(s, "fixed", out)


def test_svision_takes_sam_text_under_the_switch(checkpoint, tmp_path):
    """SVX_DEVICE_SORT=write ./SVision -b x.sam: OUT/x.sorted.bam + .bai, then the VCF and segments/ of the run on the pre-sorted BAM;
    without the switch the text is refused."""
    path, sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), tmp_path, 21)
    table = bam.read_bam(path, with_seq=True)
    refs = list(zip(table.references, table.lengths))
    sam_path = str(tmp_path / "collect_small.sam")
    with open(sam_path, "wb") as f:
        f.write(samtext.text(refs, samtext.records_of_table(table), header=table.header_text))
    fasta = helpers.load_golden_fasta("collect_small.fa.gz")
    fa = str(tmp_path / "collect_small.fa")
    bam.write_fasta(fa, {n: fasta._seq[n] for n in fasta.references})
    args = ["-m", checkpoint, "-g", fa, "-n", "HGs", "-s", "3", "--window_size", "150000", "--batch_size", "64", "--debug", "-t", "1"]
    outs = {}
    for what, src, env in (("sorted", sorted_path, {}), ("sam", sam_path, {"SVX_DEVICE_SORT": "write"}), ("refused", sam_path, {})):
        out = str(tmp_path / ("out_" + what))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "SVision"), "-o", out, "-b", src] + args, capture_output=True, text=True, timeout=900,
                           env=_env(dict(env, SVX_TIMING="1")))
        if what == "refused":
            assert r.returncode != 0 and not os.path.exists(os.path.join(out, "collect_small.sorted.bam"))
            continue
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        seg = os.path.join(out, "segments")
        outs[what] = (open(os.path.join(out, "HGs.svision.s3.vcf"), "rb").read(), {f: open(os.path.join(seg, f), "rb").read() for f in sorted(os.listdir(seg))})
    written = os.path.join(str(tmp_path / "out_sam"), "collect_small.sorted.bam")
    assert os.path.exists(written) and os.path.exists(written + ".bai")
    assert outs["sorted"][0].count(b"\n") > 20 and outs["sam"] == outs["sorted"]
