"""A sample straight from what an aligner writes (svision_amd/ingest_sort.py under SVX_DEVICE_SORT=1): load_sample on SAM text, on
the same text through a FIFO and on lists of BAM / SAM inputs against load_sample on the same records as ONE unsorted BAM -- every
table array, the name list, the bases, the scan --; the refusals, each one line that leaves nothing behind; and the command line
against its run on the sorted, indexed file and under SVX_DEVICE_SORT=write."""
import gzip
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from svision_amd.io import bam
from tests import helpers, htslike, sam_cases, sam_pack_cases as pc, samtext, sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_SV = 50
CHUNKS = (4 << 10, 64 << 10, None)                              # ``range_bytes``: many chunks and lines longer than one, a few, the default
NO_FASTA = bam.Fasta(sequences={"chrA": b"ACGT"})


def _load(src, with_seq=True, range_bytes=None, stats=None, fasta=NO_FASTA):
    from svision_amd import ingest_sort
    return ingest_sort.load_sample(src, fasta, MIN_SV, device=DEV, with_seq=with_seq, range_bytes=range_bytes, stats=stats)


def _same(got, want, with_seq=True, what=""):
    """Table array for table array, the name list, the bases, and the Sample's scan outputs."""
    sortcases.assert_same_table(got.table, want.table, with_seq=with_seq, what=what)
    assert (got.table.seq_packed is None) == (not with_seq)
    assert np.array_equal(got.gap_off, want.gap_off) and np.array_equal(got.stats, want.stats), what
    assert got.gaps.dtype == want.gaps.dtype and got.gaps.tobytes() == want.gaps.tobytes(), what
    assert np.array_equal(got.table.ref_span, want.table.ref_span), what


def _synth(ont, seed):
    from svision_amd import synth
    cfg = synth.SimConfig(contigs=[("chrA", 300_000), ("chrB", 200_000)], coverage=2.0, seed=seed)
    if ont:
        cfg.lognormal, cfg.read_len_mean, cfg.err_rate = True, 12_000.0, 0.06
    table, _genome, _svs = synth.simulate(cfg, with_seq=True)
    rng = np.random.default_rng(seed)
    recs = samtext.records_of_table(table, rng, tags=True)
    return list(zip(table.references, table.lengths)), [recs[i] for i in rng.permutation(len(recs))]


def _write(d, name, refs, recs, header=None, last_newline=True):
    """The records as SAM text and as an unsorted BAM of the test-side writer -> (text path, its bytes, BAM path)."""
    header = samtext.header_text(refs) if header is None else header
    text = header.encode("latin-1") + b"".join(samtext.line(r, refs) + b"\n" for r in recs)
    text = text if last_newline else text[:-1]
    path = os.path.join(d, name + ".sam")
    with open(path, "wb") as f:
        f.write(text)
    bam_path = os.path.join(d, name + ".bam")
    htslike.write_bam(bam_path, refs, [samtext.for_htslike(r) for r in recs], level=1, policy="stream", header_text=header, index=False)
    return path, text, bam_path


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """name -> dict(sam, text, bam, want: load_sample(the BAM) with bases, want_plain: without, fasta): written and loaded once."""
    d = str(tmp_path_factory.mktemp("sort_inputs"))
    out = {}
    shuffled, _sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), d, 21)
    table = bam.read_bam(shuffled, with_seq=True)
    refs = list(zip(table.references, table.lengths))
    recs = samtext.records_of_table(table, np.random.default_rng(3), tags=True)
    # (the golden file's odd-length reads carry a set spare nibble, which text cannot express: the BAM of the text's records is compared)
    sam_path, text, bam_path = _write(d, "collect_small.text", refs, recs, header=table.header_text)
    out["collect_small"] = dict(sam=sam_path, text=text, bam=bam_path, shuffled=shuffled, fasta=helpers.load_golden_fasta("collect_small.fa.gz"),
                                n=len(recs))
    for name, (refs, recs) in (("hifi", _synth(False, 5)), ("ont", _synth(True, 6))):
        sam_path, text, bam_path = _write(d, name, refs, recs, last_newline=name != "ont")
        out[name] = dict(sam=sam_path, text=text, bam=bam_path, fasta=NO_FASTA, n=len(recs))
    # the case list, the host's line in its middle
    host_line, _words = pc.placeholder_line()
    recs = sam_cases.records()
    at = len(recs) // 2
    host_rec = dict(qname="long_cigar", tid=1, pos=4242, flag=0, mapq=60, cigar=[(10, "S"), (sum(1 + i % 5 for i in range(70) if i % 3 != 1), "N")],
                    seq="ACGTACGTAC", qual=bytes(10), tags=[("NM", "i", 5), ("CG", "BI", _words), ("XZ", "Z", "behind")])
    assert samtext.line(host_rec, pc.REFS) == host_line
    recs = recs[:at] + [host_rec] + recs[at:]
    sam_path, text, bam_path = _write(d, "cases", pc.REFS, recs)
    out["cases"] = dict(sam=sam_path, text=text, bam=bam_path, fasta=NO_FASTA, n=len(recs))
    for name, s in out.items():
        s["dir"] = d
        s["want"], s["want_plain"] = _load(s["bam"], True, fasta=s["fasta"]), _load(s["bam"], False, fasta=s["fasta"])
        assert len(s["want"].table) == s["n"]
    assert out["hifi"]["n"] > 30 and out["ont"]["n"] > 20 and len(out["collect_small"]["want"].gaps) > 0
    return out


class Fifo:
    """A FIFO in ``d`` that a daemon thread writes ``data`` into, ``step`` bytes a write (None: at once), the bytes in front of
    ``cut`` in a write of their own (BrokenPipeError noted: the reader may close early)."""

    def __init__(self, d, data, step=None, cut=0, name="fifo"):
        self.path, self.broke = os.path.join(str(d), name), False
        os.mkfifo(self.path)

        def feed():
            try:
                with open(self.path, "wb", buffering=0) as f:
                    pieces = ([data[:cut]] if cut else []) + [data[at:at + (step or len(data))] for at in range(cut, len(data), step or max(len(data), 1))]
                    for piece in pieces:
                        while piece:                            # (a raw write may be cut short by a reader that closes: the next one says so)
                            piece = piece[f.write(piece):]
            except BrokenPipeError:
                self.broke = True
        self.thread = threading.Thread(target=feed, daemon=True)
        self.thread.start()

    def done(self):
        self.thread.join(30)
        ended = not self.thread.is_alive()
        os.unlink(self.path)
        return ended


# ---- 1. text in a file ----
@pytest.mark.parametrize("range_bytes", CHUNKS, ids=["4K", "64K", "default"])
@pytest.mark.parametrize("name", ["collect_small", "hifi", "ont", "cases"])
def test_text_equals_the_unsorted_bam(sets, name, range_bytes):
    from svision_amd import ingest_sort
    s, stats = sets[name], {}
    _same(_load(s["sam"], True, range_bytes, stats, s["fasta"]), s["want"], True, name)
    assert stats["inputs"] == ["sam"] and stats["records"] == s["n"] and stats["host_lines"] == (1 if name == "cases" else 0)
    assert set(stats["seconds"]) == set(ingest_sort.STAGES) and stats["seconds"]["pack"] > 0 and stats["seconds"]["walk"] == 0
    assert stats["ranges"] == 1 if range_bytes is None else stats["ranges"] > (3 if range_bytes == 4 << 10 else 0)
    if range_bytes == 4 << 10:
        _same(_load(s["sam"], False, range_bytes, None, s["fasta"]), s["want_plain"], False, name)


def test_the_bam_road_reports_its_kind(sets):
    stats = {}
    _load(sets["collect_small"]["bam"], False, None, stats, sets["collect_small"]["fasta"])
    assert stats["inputs"] == ["bam"] and stats["host_lines"] == 0 and stats["seconds"]["pack"] == 0 and stats["seconds"]["lines"] == 0


# ---- 2. text through a pipe ----
@pytest.mark.parametrize("step", [1, 7, 64 << 10, None], ids=["1", "7", "64K", "at_once"])
def test_a_fifo_equals_the_file(sets, tmp_path, step):
    """Small writes on a small text (every read boundary, the header's end among them), large ones on the larger sets."""
    if step in (1, 7):
        s = sets["collect_small"]
        lines = s["text"].split(b"\n")
        n_head = sum(l.startswith(b"@") for l in lines)
        text = b"\n".join(lines[:n_head + 12]) + b"\n"
        path = str(tmp_path / "small.sam")
        with open(path, "wb") as f:
            f.write(text)
        want = _load(path, True, 4 << 10, fasta=s["fasta"])
        for cut in (0, len(b"\n".join(lines[:n_head])) + 1):   # the header in a write of its own: it ends at a read boundary
            fifo, stats = Fifo(tmp_path, text, step, cut), {}
            _same(_load(fifo.path, True, 4 << 10, stats, s["fasta"]), want, True, "small")
            assert fifo.done() and stats["inputs"] == ["pipe"] and stats["records"] == 12
        return
    for name in ("hifi", "ont", "cases"):
        s = sets[name]
        fifo, stats = Fifo(tmp_path, s["text"], step), {}
        _same(_load(fifo.path, True, 64 << 10, stats, s["fasta"]), s["want"], True, name)
        assert fifo.done() and not fifo.broke and stats["inputs"] == ["pipe"] and stats["ranges"] > 3
        assert stats["host_lines"] == (1 if name == "cases" else 0)


# ---- 3. several inputs ----
REFS_A = [("chrA", 1_000_000), ("chrB", 500_000)]
REFS_B = [("chrC", 300_000), ("chrA", 1_000_000)]
MERGED = REFS_A + [REFS_B[0]]


def _records(prefix, names, n, seed):
    """n records on the references ``names``; positions from a few values, so that records tie within and across inputs."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        l = int(rng.integers(1, 40))
        unplaced = i % 11 == 3
        out.append(dict(qname="%s%d" % (prefix, i), ref=None if unplaced else names[int(rng.integers(0, len(names)))],
                        pos=-1 if unplaced else int(rng.choice([0, 7, 7, 100, 4096, 250_000])), flag=4 if unplaced else (0, 16)[i & 1],
                        mapq=int(rng.integers(0, 61)), cigar=[] if unplaced else [(l, "M"), (int(rng.integers(50, 90)), "D"), (3, "M")],
                        seq="".join("ACGT"[int(b)] for b in rng.integers(0, 4, l + 3)), qual=None, tags=[("NM", "i", i)]))
    return out


def _numbered(recs, refs):
    names = [r[0] for r in refs]
    return [dict(r, tid=-1 if r["ref"] is None else names.index(r["ref"])) for r in recs]


@pytest.fixture(scope="module")
def parts(tmp_path_factory):
    """dictionaries -> (the list of a.bam, b.sam and the headerless c.sam in ``order``, b.sam's text, load_sample of the one unsorted
    BAM under the merged header).  ``bam_second``: the BAM behind b.sam, so its tids go through a table that is not the identity."""
    d = str(tmp_path_factory.mktemp("sort_inputs_parts"))
    out = {}
    for what, refs_b, merged, order in (("identical", REFS_A, REFS_A, "abc"), ("renumbered", REFS_B, MERGED, "abc"),
                                        ("bam_second", REFS_B, REFS_B + [REFS_A[1]], "bac")):
        recs = {"a": _records("a", ["chrA", "chrB"], 70, 1), "b": _records("b", [r[0] for r in refs_b], 60, 2),
                "c": _records("c", [merged[-1][0], "chrA"], 50, 3)}
        _sam, _text, a_bam = _write(d, what + ".a", REFS_A, _numbered(recs["a"], REFS_A))
        b_sam, b_text, _bam = _write(d, what + ".b", refs_b, _numbered(recs["b"], refs_b))
        c_sam, _text, _bam = _write(d, what + ".c", merged, _numbered(recs["c"], merged), header="@CO\tno dictionary here\n")
        _sam, _text, one = _write(d, what + ".one", merged, _numbered([r for p in order for r in recs[p]], merged))
        out[what] = dict(paths=[{"a": a_bam, "b": b_sam, "c": c_sam}[p] for p in order], b_text=b_text, want=_load(one), merged=merged, n=180,
                         order=order, kinds=[{"a": "bam", "b": "sam", "c": "sam"}[p] for p in order])
    return out


@pytest.mark.parametrize("what", ["identical", "renumbered", "bam_second"])
def test_a_list_equals_the_one_bam(parts, what, tmp_path):
    p, stats = parts[what], {}
    got = _load(p["paths"], True, 4 << 10, stats)
    _same(got, p["want"], True, what)
    assert stats["inputs"] == p["kinds"] and stats["records"] == p["n"]
    assert list(zip(got.table.references, got.table.lengths)) == p["merged"]
    # records that tie across the inputs: list order, then file order
    t = got.table
    key = sortcases.key(t.tid, t.pos, len(p["merged"]))
    tied = [[t.names[int(t.name_id[i])] for i in np.flatnonzero(key == k)] for k in np.unique(key)]
    assert any(len({n[0] for n in names}) == 3 for names in tied)
    for names in tied:
        assert names == sorted(names, key=lambda n: (p["order"].index(n[0]), int(n[1:]))), names
    # a pipe as one of the parts, and a tuple for the list
    fifo = Fifo(tmp_path, p["b_text"], 4096)
    with_pipe = tuple(fifo.path if k == p["order"].index("b") else path for k, path in enumerate(p["paths"]))
    _same(_load(with_pipe, True, None, stats), p["want"], True, what + " with a pipe")
    assert fifo.done() and stats["inputs"] == ["pipe" if k == "sam" and i == p["order"].index("b") else k for i, k in enumerate(p["kinds"])]


# ---- 4. refusals ----
def _refused(src, match, d, **kw):
    from svision_amd import ingest_sort
    before = sorted(os.listdir(str(d)))
    with pytest.raises(ingest_sort.SortIngestError, match=match) as exc:
        _load(src, **kw)
    assert "\n" not in str(exc.value) and sorted(os.listdir(str(d))) == before
    return str(exc.value)


def test_refusals(sets, parts, tmp_path):
    s = sets["hifi"]
    lines = s["text"].split(b"\n")
    n_head = sum(l.startswith(b"@") for l in lines)
    body = [l for l in lines[n_head:] if l]
    # a bad line in the third chunk of a pipe: its number, and the writer ended although most of its text was never read
    short = [samtext.line(dict(sam_cases.records()[3], qname="s%d" % i), [("chrA", 300_000)]) for i in range(100_000)]
    head = b"\n".join(lines[:n_head]) + b"\n"
    chunk = 4 << 10
    good, size = [], 0
    while size < 2 * chunk + 100:
        good.append(short[len(good)])
        size += len(good[-1]) + 1
    bad = short[0].replace(b"\t60\t", b"\t6x\t")
    text = head + b"\n".join(good + [bad] + short[len(good):]) + b"\n"
    assert len(text) > 2 << 20
    fifo = Fifo(tmp_path, text)
    said = _refused(fifo.path, "line %d: MAPQ" % (n_head + len(good) + 1), tmp_path, range_bytes=chunk)
    assert said.startswith(fifo.path + ": ") and fifo.done() and fifo.broke
    # a BAM and gzip data on a pipe
    fifo = Fifo(tmp_path, open(s["bam"], "rb").read())
    assert "pipe" in _refused(fifo.path, "SVX_DEVICE_SORT=write", tmp_path) and fifo.done()
    fifo = Fifo(tmp_path, gzip.compress(s["text"]))
    _refused(fifo.path, "pigz -dc", tmp_path)
    assert fifo.done()
    # a single SAM without a dictionary; an RNAME in no dictionary; standard input twice
    _refused(parts["renumbered"]["paths"][2], "@SQ", tmp_path)
    unknown = str(tmp_path / "unknown.sam")
    with open(unknown, "wb") as f:
        f.write(head + b"\n".join(body[:5] + [body[5].replace(b"\tchr", b"\tnot_chr", 1)] + body[6:9]) + b"\n")
    said = _refused(unknown, "line %d: the reference 'not_chr" % (n_head + 6), tmp_path)
    assert said.startswith(unknown + ": ")
    os.unlink(unknown)
    _refused(["-", "-"], "named twice", tmp_path)
    _refused([parts["renumbered"]["paths"][0], "-", "-"], "named twice", tmp_path)


# ---- 5. the command line (child processes: what the test is about) ----
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


def test_svision_calls_from_text_a_pipe_and_a_list(sets, checkpoint, tmp_path):
    """SVX_DEVICE_SORT=1 ./SVision -b text.sam | -b - | -b a.bam,b.sam | -b <a FIFO>: the VCF and segments/ of the run on the pre-sorted, indexed
    BAM and of SVX_DEVICE_SORT=write on the same text; no alignment file appears in OUT/."""
    s = sets["collect_small"]
    sorted_path = os.path.join(s["dir"], "collect_small.sorted.bam")
    lines = s["text"].split(b"\n")
    n_head = sum(l.startswith(b"@") for l in lines)
    half = n_head + (len(lines) - n_head) // 2
    table = bam.read_bam(s["shuffled"], with_seq=True)
    first_half = str(tmp_path / "first_half.bam")
    bam.write_bam(first_half, table.subset(np.arange(half - n_head)), with_seq=True, index=False)
    second_half = str(tmp_path / "second_half.sam")
    with open(second_half, "wb") as f:
        f.write(b"\n".join(lines[:n_head] + lines[half:]))
    fa = str(tmp_path / "collect_small.fa")
    bam.write_fasta(fa, {n: s["fasta"]._seq[n] for n in s["fasta"].references})
    args = ["-m", checkpoint, "-g", fa, "-n", "HGs", "-s", "3", "--window_size", "150000", "--batch_size", "64", "--debug"]
    runs = (("sorted", sorted_path, {}, "1"), ("write", s["sam"], {"SVX_DEVICE_SORT": "write"}, "1"), ("text", s["sam"], {"SVX_DEVICE_SORT": "1"}, "1"),
            ("stdin", "-", {"SVX_DEVICE_SORT": "1"}, "1"), ("list", first_half + "," + second_half, {"SVX_DEVICE_SORT": "1"}, "1"),
            ("fifo", "a FIFO", {"SVX_DEVICE_SORT": "1"}, "1"), ("text_t3", s["sam"], {"SVX_DEVICE_SORT": "1"}, "3"))
    outs = {}
    for what, src, env, threads in runs:
        out = str(tmp_path / ("out_" + what))
        fifo = Fifo(tmp_path, s["text"], name="aligner.fifo") if what == "fifo" else None     # (-b <a path that is no regular file>: read once, as ``-``)
        src = fifo.path if fifo else src
        r = subprocess.run([sys.executable, os.path.join(ROOT, "SVision"), "-o", out, "-b", src, "-t", threads] + args,
                           input=s["text"] if src == "-" else None, capture_output=True, timeout=900, env=_env(dict(env, SVX_TIMING="1")))
        assert r.returncode == 0, (what, r.stdout.decode()[-2000:] + r.stderr.decode()[-3000:])
        assert fifo is None or (fifo.done() and not fifo.broke)
        seg = os.path.join(out, "segments")
        outs[what] = (open(os.path.join(out, "HGs.svision.s3.vcf"), "rb").read(), {f: open(os.path.join(seg, f), "rb").read() for f in sorted(os.listdir(seg))})
        if env.get("SVX_DEVICE_SORT") == "1":
            assert not [f for _dir, _sub, names in os.walk(out) for f in names if f.endswith((".bam", ".bai")) or ".spool." in f], what
    assert outs["sorted"][0].count(b"\n") > 20
    for what in ("write", "text", "stdin", "list", "fifo", "text_t3"):
        assert outs[what] == outs["sorted"], what
