"""sort_bam on an aligner's output that arrives through a pipe (svision_amd/sort_sources.py: PipeSource over io.sam.StreamReader): the text is
seen ONCE -- measured and encoded chunk by chunk into a record stream that grows on the device, or, beyond the budget, spooled as an
unsorted BAM beside the output -- and the two files written must be, byte for byte, those of the same bytes read from a regular file.
The sets are the shuffled HiFi- and ONT-shaped ones of tests/test_gpu_sort_sam.py (a few hundred records) and the case list of
tests/sam_cases.py (host-encoded lines, lines longer than a chunk).  In-process tests read a FIFO fed by a daemon thread; the
command lines get the text on their standard input."""
import gzip
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from svision_amd.io import bam
from tests import helpers, htslike, sam_cases, samtext, sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (4 << 10, 64 << 10)                                    # ``range_bytes``: many chunks, carried lines, lines longer than a chunk


def _synth_records(ont, seed):
    from svision_amd import synth
    cfg = synth.SimConfig(contigs=[("chrA", 900_000), ("chrB", 600_000)], coverage=2.5, seed=seed)
    if ont:
        cfg.lognormal, cfg.read_len_mean, cfg.err_rate, cfg.coverage = True, 12_000.0, 0.06, 2.0
    table, _genome, _svs = synth.simulate(cfg, with_seq=True)
    rng = np.random.default_rng(seed)
    recs = samtext.records_of_table(table, rng, tags=True)
    return list(zip(table.references, table.lengths)), [recs[i] for i in rng.permutation(len(recs))]


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """name -> dict(sam: the text as a regular file; text: its bytes; n: records; host_lines; want: per tables the two files that
    sort_bam(the regular file) writes; room: the records' bytes): written and sorted once, left unchanged."""
    from svision_amd import sort
    d = str(tmp_path_factory.mktemp("sort_pipe"))
    out = {}
    for name, (refs, recs), host_lines in (("cases", (sam_cases.REFS, sam_cases.records()), len(sam_cases.refused_lines())),
                                           ("hifi", _synth_records(False, 5), 0), ("ont", _synth_records(True, 6), 0)):
        path = os.path.join(d, name + ".sam")
        text = samtext.text(refs, recs, header=samtext.header_text(refs), last_newline=name != "ont")
        with open(path, "wb") as f:
            f.write(text)
        s = out[name] = dict(sam=path, text=text, n=len(recs), host_lines=host_lines, refs=refs, recs=recs, dir=d, want={})
        for tables in ("fixed", "dynamic") if name != "cases" else ("fixed",):
            p, stats = os.path.join(d, "%s.%s.from_file.bam" % (name, tables)), {}
            sort.sort_bam(path, p, device=DEV, tables=tables, stats=stats)
            assert "pipe" not in stats
            s["want"][tables] = (open(p, "rb").read(), open(p + ".bai", "rb").read())
            s["room"] = stats["stream_bytes"] - 4
    assert out["hifi"]["n"] > 150 and out["ont"]["n"] > 100
    return out


class Fifo:
    """A FIFO in ``d`` that a daemon thread writes ``data`` into (BrokenPipeError ignored: the reader may close early)."""

    def __init__(self, d, data, name="fifo"):
        self.path, self.broke = os.path.join(str(d), name), False
        os.mkfifo(self.path)

        def feed():
            try:
                with open(self.path, "wb") as f:
                    f.write(data)
            except BrokenPipeError:
                self.broke = True
        self.thread = threading.Thread(target=feed, daemon=True)
        self.thread.start()

    def done(self):
        self.thread.join(30)
        ended = not self.thread.is_alive()
        os.unlink(self.path)
        return ended


def _same_files(want, path):
    assert open(path, "rb").read() == want[0]
    assert open(path + ".bai", "rb").read() == want[1]
    assert not [n for n in os.listdir(os.path.dirname(path)) if n.endswith(".tmp") or ".spool." in n]


@pytest.mark.parametrize("range_bytes", CHUNKS, ids=["4K", "64K"])
@pytest.mark.parametrize("tables", ["fixed", "dynamic"])
@pytest.mark.parametrize("name", ["hifi", "ont"])
def test_a_pipe_gives_the_files_of_the_file_road(sets, name, tables, range_bytes, tmp_path):
    from svision_amd import sort
    s = sets[name]
    fifo = Fifo(tmp_path, s["text"])
    out, stats = str(tmp_path / "out.bam"), {}
    assert sort.sort_bam(fifo.path, out, device=DEV, tables=tables, range_bytes=range_bytes, stats=stats) == out
    assert fifo.done()
    _same_files(s["want"][tables], out)
    pipe = stats["pipe"]
    assert pipe["mode"] == "in_core" and pipe["spool_bytes"] == 0 and pipe["text_bytes"] == len(s["text"])
    assert stats["input"] == "sam" and stats["records"] == s["n"] and stats["spans"] == 1 and stats["host_lines"] == 0
    assert set(stats["seconds"]) == set(sort.STAGES)
    assert stats["ranges"] > 4 and pipe["grows"] == stats["ranges"] + 1          # a segment a chunk, and the join
    # (a): within the budget; (b): within twice the record bytes seen plus one chunk's records -- the join's two copies and the slack
    assert stats["stream_bytes"] <= stats["memory_bytes"]
    assert stats["stream_bytes"] == 2 * s["room"] + 4 and stats["stream_bytes"] <= 2 * s["room"] + _last_chunk_records(s, stats)


def _last_chunk_records(s, stats):
    """The record bytes of the pass's last chunk: the lengths of the last ``range_records[-1]`` lines' records, by io.sam."""
    from svision_amd.io import sam
    tid_of = sam.tid_table([r for r, _n in s["refs"]])
    lines = [l for l in s["text"].split(b"\n") if l and not l.startswith(b"@")]
    return sum(len(sam.encode_line(l, tid_of)) for l in lines[-stats["range_records"][-1]:])


def test_host_encoded_lines_and_lines_longer_than_a_chunk(sets, tmp_path):
    from svision_amd import sort
    s = sets["cases"]
    for range_bytes in CHUNKS:
        fifo = Fifo(tmp_path, s["text"])
        out, stats = str(tmp_path / ("cases%d.bam" % range_bytes)), {}
        sort.sort_bam(fifo.path, out, device=DEV, range_bytes=range_bytes, stats=stats)
        assert fifo.done()
        _same_files(s["want"]["fixed"], out)
        assert stats["pipe"]["mode"] == "in_core" and stats["host_lines"] == s["host_lines"] > 0 and stats["records"] == s["n"]


@pytest.mark.parametrize("name", ["hifi", "ont"])
def test_beyond_the_budget_the_pipe_is_spooled(sets, name, tmp_path):
    from svision_amd import sort
    s = sets[name]
    for what, budget in (("a_fifth", s["room"] // 5), ("one_byte", 1)):
        fifo = Fifo(tmp_path, s["text"])
        out, stats = str(tmp_path / (what + ".bam")), {}
        sort.sort_bam(fifo.path, out, device=DEV, memory_bytes=budget, range_bytes=CHUNKS[1], stats=stats)
        assert fifo.done()
        _same_files(s["want"]["fixed"], out)
        pipe = stats["pipe"]
        assert pipe["mode"] == "spooled" and pipe["spool_bytes"] > 0 and stats["spans"] > 1 and stats["input"] == "sam"
        assert stats["records"] == s["n"] and stats["host_lines"] == 0
        assert sorted(os.listdir(str(tmp_path))) == sorted(os.path.basename(out) + e for e in ("", ".bai"))
        for n in os.listdir(str(tmp_path)):
            os.unlink(str(tmp_path / n))


def test_the_spool_takes_the_kept_records_first_and_the_hosts_lines(sets, tmp_path):
    """A budget that holds some chunks and not all: what was kept goes into the spool in front of the later chunks; the case list
    brings lines the host encodes, on both sides of the switch."""
    from svision_amd import sort
    s = sets["cases"]
    fifo = Fifo(tmp_path, s["text"])
    out, stats = str(tmp_path / "out.bam"), {}
    sort.sort_bam(fifo.path, out, device=DEV, memory_bytes=s["room"], range_bytes=CHUNKS[0], stats=stats)
    assert fifo.done()
    _same_files(s["want"]["fixed"], out)
    assert stats["pipe"]["mode"] == "spooled" and stats["pipe"]["grows"] > 1 and stats["host_lines"] == s["host_lines"]


def test_header_only_and_no_byte_and_compressed_text(sets, tmp_path):
    from svision_amd import sort
    text = samtext.header_text(sam_cases.REFS[:3]).encode()
    path = str(tmp_path / "empty.sam")
    with open(path, "wb") as f:
        f.write(text)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    sort.sort_bam(path, a, device=DEV)
    fifo, stats = Fifo(tmp_path, text), {}
    sort.sort_bam(fifo.path, b, device=DEV, stats=stats)
    assert fifo.done()
    assert open(a, "rb").read() == open(b, "rb").read() and open(a + ".bai", "rb").read() == open(b + ".bai", "rb").read()
    assert stats["records"] == 0 and stats["input"] == "sam" and stats["pipe"]["mode"] == "in_core"
    before = sorted(os.listdir(str(tmp_path)))
    for data, match in ((b"", "no input"), (gzip.compress(sets["hifi"]["text"][:1 << 16]), "compressed SAM is not taken")):
        fifo = Fifo(tmp_path, data)
        with pytest.raises(sort.SortWriteError, match=match):
            sort.sort_bam(fifo.path, str(tmp_path / "never.bam"), device=DEV)
        assert fifo.done() and sorted(os.listdir(str(tmp_path))) == before


@pytest.mark.parametrize("budget", [None, 1], ids=["in_core", "spooled"])
def test_a_bad_line_in_the_third_chunk(sets, budget, tmp_path):
    """The error names the stream's line; nothing is left behind; the feeding thread has ended although most of the text was never
    read: the read end was closed."""
    from svision_amd import sort
    s = sets["hifi"]
    lines = s["text"].split(b"\n")
    n_head = sum(l.startswith(b"@") for l in lines)
    at, k = 0, n_head
    while at < 2 * CHUNKS[0] + 100:                             # the first line that lies wholly in the third chunk or behind it
        at += len(lines[k]) + 1
        k += 1
    cols = lines[k + 1].split(b"\t")
    cols[3] = b"12x"
    lines[k + 1] = b"\t".join(cols)
    text = b"\n".join(lines) * 8                                # (far more than a pipe holds: the writer blocks until the read end closes)
    assert len(text) > 1 << 20
    fifo = Fifo(tmp_path, text)
    before = sorted(os.listdir(str(tmp_path)))
    with pytest.raises(sort.SortWriteError, match=r"line %d: POS is not a number" % (k + 2)) as exc:
        sort.sort_bam(fifo.path, str(tmp_path / "never.bam"), device=DEV, range_bytes=CHUNKS[0], memory_bytes=budget)
    assert fifo.path in str(exc.value)
    assert sorted(os.listdir(str(tmp_path))) == before
    assert fifo.done() and fifo.broke


def test_a_bam_on_a_pipe_is_spooled_as_it_is(sets, tmp_path):
    from svision_amd import sort
    s = sets["hifi"]
    path = str(tmp_path / "in.bam")
    htslike.write_bam(path, s["refs"], [samtext.for_htslike(r) for r in s["recs"]], level=1, policy="stream", header_text=samtext.header_text(s["refs"]),
                      index=False)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    sort.sort_bam(path, a, device=DEV)
    fifo, stats = Fifo(tmp_path, open(path, "rb").read()), {}
    sort.sort_bam(fifo.path, b, device=DEV, stats=stats)
    assert fifo.done()
    _same_files((open(a, "rb").read(), open(a + ".bai", "rb").read()), b)
    assert stats["pipe"]["mode"] == "bam_spooled" and stats["pipe"]["spool_bytes"] == os.path.getsize(path) and "input" not in stats
    assert open(a, "rb").read() == s["want"]["fixed"][0]


def test_a_pipe_among_several_inputs(sets, tmp_path):
    """[a.bam, fifo, c.sam] == [a.bam, the text as a file, c.sam]; every part has records at the same (reference, position): ties come
    out in list order.  The pipe has no @SQ line: the other parts' dictionary serves it."""
    from svision_amd import sort
    s = sets["hifi"]
    refs, recs = s["refs"], s["recs"][:120]
    parts = [[dict(r, qname="%s_%d" % (r["qname"], k)) for r in recs] for k in range(3)]
    header = samtext.header_text(refs)
    a, mid, c = str(tmp_path / "a.bam"), str(tmp_path / "mid.sam"), str(tmp_path / "c.sam")
    htslike.write_bam(a, refs, [samtext.for_htslike(r) for r in parts[0]], level=1, policy="stream", header_text=header, index=False)
    mid_text = samtext.text(refs, parts[1], header="")
    assert not mid_text.startswith(b"@")
    for path, text in ((mid, mid_text), (c, samtext.text(refs, parts[2], header=header))):
        with open(path, "wb") as f:
            f.write(text)
    want, got = str(tmp_path / "want.bam"), str(tmp_path / "got.bam")
    sort.sort_bam([a, mid, c], want, device=DEV)
    fifo, stats = Fifo(tmp_path, mid_text), {}
    sort.sort_bam([a, fifo.path, c], got, device=DEV, range_bytes=CHUNKS[1], stats=stats)
    assert fifo.done()
    _same_files((open(want, "rb").read(), open(want + ".bai", "rb").read()), got)
    assert stats["pipe"]["mode"] == "spooled" and stats["inputs"] == 3 and stats["input_records"] == [120, 120, 120] and stats["retid_inputs"] == 0
    table = bam.read_bam(got)
    where = {}
    for i, nid in enumerate(table.name_id):                     # every read's three copies have one key: part 0, 1, 2 in that order
        stem, k = table.names[int(nid)].rsplit("_", 1)
        where.setdefault(stem, {})[int(k)] = i
    assert len(where) == 120 and all(w[0] < w[1] < w[2] for w in where.values())
    before = sorted(os.listdir(str(tmp_path)))
    with pytest.raises(sort.SortWriteError, match="named twice"):
        sort.sort_bam([a, "-", "-"], str(tmp_path / "never.bam"), device=DEV)
    assert sorted(os.listdir(str(tmp_path))) == before


def test_two_pipes_in_one_list_are_both_reported(sets, tmp_path):
    """Two FIFOs (only ``-`` is limited to one): the files of the same two texts as regular files; ``stats["pipes"]`` has both."""
    from svision_amd import sort
    s = sets["hifi"]
    header = samtext.header_text(s["refs"])
    texts = [samtext.text(s["refs"], s["recs"][:60], header=header), samtext.text(s["refs"], s["recs"][60:100], header=header)]
    paths = []
    for k, text in enumerate(texts):
        paths.append(str(tmp_path / ("part%d.sam" % k)))
        with open(paths[-1], "wb") as f:
            f.write(text)
    want, got = str(tmp_path / "want.bam"), str(tmp_path / "got.bam")
    sort.sort_bam(paths, want, device=DEV)
    fifos, stats = [Fifo(tmp_path, text, "fifo%d" % k) for k, text in enumerate(texts)], {}
    sort.sort_bam([f.path for f in fifos], got, device=DEV, range_bytes=CHUNKS[1], stats=stats)
    assert all(f.done() for f in fifos)
    _same_files((open(want, "rb").read(), open(want + ".bai", "rb").read()), got)
    assert [(p["name"], p["mode"], p["text_bytes"]) for p in stats["pipes"]] == [(f.path, "spooled", len(t)) for f, t in zip(fifos, texts)]
    assert stats["pipe"] == {k: v for k, v in stats["pipes"][0].items() if k != "name"} and stats["input"] == "sam"
    assert stats["input_records"] == [60, 40]


# ---- the command lines (child processes with the text on standard input: what the tests are about) ----
def _env(extra):
    base = {k: v for k, v in os.environ.items() if k not in ("SVX_DEVICE_SORT", "SVX_BUILD_INDEX", "SVX_INGEST", "SVX_SORT_TABLES", "SVX_SORT_MEMORY")}
    return dict(base, PYTHONPATH=ROOT, **extra)


def test_module_command_line_on_standard_input(sets, tmp_path):
    s = sets["hifi"]
    out = str(tmp_path / "cli.bam")
    r = subprocess.run([sys.executable, "-m", "svision_amd.sort", "-", "-o", out], input=s["text"], capture_output=True, timeout=600, env=_env({}),
                       cwd=str(tmp_path))
    stdout, stderr = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0 and "%d records" % s["n"] in stdout and "<stdin>" in stdout and "kept in core" in stdout, stdout[-2000:] + stderr[-3000:]
    _same_files(s["want"]["fixed"], out)
    # a failing line: exit status 1, one line on stderr, nothing written
    lines = s["text"].split(b"\n")
    k = next(i for i, l in enumerate(lines) if not l.startswith(b"@")) + 5
    lines[k] = b"\t".join(lines[k].split(b"\t")[:10])
    before = sorted(os.listdir(str(tmp_path)))
    r = subprocess.run([sys.executable, "-m", "svision_amd.sort", "-", "-o", str(tmp_path / "never.bam")], input=b"\n".join(lines), capture_output=True,
                       timeout=600, env=_env({}), cwd=str(tmp_path))
    err = [l for l in r.stderr.decode().strip().splitlines() if "libdrm" not in l]          # (the graphics library's own note is not the tool's)
    assert r.returncode == 1 and len(err) == 1 and "<stdin>: line %d:" % (k + 1) in err[0], r.stderr.decode()[-3000:]
    assert sorted(os.listdir(str(tmp_path))) == before


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from oracle import alexnet_ref
    from svision_amd.network import tf_checkpoint as ck
    prefix = str(tmp_path_factory.mktemp("ckpt") / "svision-cnn-model.ckpt")
    ck.write_checkpoint(prefix, alexnet_ref.random_params(seed=7))
    return prefix


def test_svision_takes_standard_input_under_the_switch(checkpoint, tmp_path):
    """SVX_DEVICE_SORT=write ./SVision -b -: OUT/stdin.sorted.bam + .bai, then the VCF and segments/ of the run on the SAM file;
    without the switch ``-b -`` is refused in one line that names it."""
    path, _sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), tmp_path, 21)
    table = bam.read_bam(path, with_seq=True)
    refs = list(zip(table.references, table.lengths))
    text = samtext.text(refs, samtext.records_of_table(table), header=table.header_text)
    sam_path = str(tmp_path / "collect_small.sam")
    with open(sam_path, "wb") as f:
        f.write(text)
    fasta = helpers.load_golden_fasta("collect_small.fa.gz")
    fa = str(tmp_path / "collect_small.fa")
    bam.write_fasta(fa, {n: fasta._seq[n] for n in fasta.references})
    args = ["-m", checkpoint, "-g", fa, "-n", "HGs", "-s", "3", "--window_size", "150000", "--batch_size", "64", "--debug", "-t", "1"]
    outs = {}
    for what, src, env in (("file", sam_path, {"SVX_DEVICE_SORT": "write"}), ("stdin", "-", {"SVX_DEVICE_SORT": "write"}), ("refused", "-", {})):
        out = str(tmp_path / ("out_" + what))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "SVision"), "-o", out, "-b", src] + args, input=text if src == "-" else None,
                           capture_output=True, timeout=900, env=_env(dict(env, SVX_TIMING="1")))
        stdout, stderr = r.stdout.decode(), r.stderr.decode()
        if what == "refused":
            logs = [os.path.join(out, f) for f in os.listdir(out) if f.startswith("SVision_") and f.endswith(".log")]
            said = [l for f in logs for l in open(f).read().splitlines() if "[ERROR" in l]         # (the run's errors go to its log file)
            assert r.returncode != 0 and len(said) == 1 and "SVX_DEVICE_SORT=write" in said[0], "\n".join(said) + stdout[-2000:] + stderr[-3000:]
            assert not os.path.exists(os.path.join(out, "stdin.sorted.bam"))
            continue
        assert r.returncode == 0, stdout[-2000:] + stderr[-3000:]
        seg = os.path.join(out, "segments")
        outs[what] = (open(os.path.join(out, "HGs.svision.s3.vcf"), "rb").read(), {f: open(os.path.join(seg, f), "rb").read() for f in sorted(os.listdir(seg))})
    written = os.path.join(str(tmp_path / "out_stdin"), "stdin.sorted.bam")
    assert os.path.exists(written) and os.path.exists(written + ".bai")
    assert open(written, "rb").read() == open(os.path.join(str(tmp_path / "out_file"), "collect_small.sorted.bam"), "rb").read()
    assert outs["file"][0].count(b"\n") > 20 and outs["stdin"] == outs["file"]
