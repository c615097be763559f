"""A sample from an unsorted BAM (svision_amd/ingest_sort.py, SVX_DEVICE_SORT=1): load_sample on record-shuffled copies of golden
files and on a file of the test-side writer (no @HD line, records across BGZF blocks, a CG-tag CIGAR, records without a reference
in the middle) against read_bam() of the stably sorted file (tests/sortcases.py: NumPy) -- every table array, the name list, the
bases, the scan --, one range and several; a corrupt block; and the command line against its run on the sorted, indexed file."""
import os
import subprocess
import sys

import numpy as np
import pytest

from svision_amd.io import bam
from svision_amd.sample import Sample
from tests import baicases, helpers, htslike, sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_SV = 50


def _htslike_files(d):
    """Unsorted records under a header without @HD, blocks cut every 0xFF00 bytes whatever the records -> (path, sorted path)."""
    recs = baicases.short_records(seed=8, n=120, cg=True)
    perm = np.random.default_rng(8).permutation(len(recs))
    shuffled = [recs[i] for i in perm]
    tids = [r["tid"] for r in shuffled]
    assert -1 in tids[10:-10] and max(len(r["cigar"]) for r in recs) > 65535
    text = "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in baicases.REFS) + "@PG\tID:aligner\tPN:aligner\n"
    path, sorted_path = os.path.join(d, "aligner.bam"), os.path.join(d, "aligner.sorted.bam")
    htslike.write_bam(path, baicases.REFS, shuffled, level=1, policy="stream", header_text=text, index=False)
    o = sortcases.order(np.asarray(tids), np.asarray([r["pos"] for r in shuffled]), len(baicases.REFS))
    htslike.write_bam(sorted_path, baicases.REFS, [shuffled[i] for i in o], level=1, policy="stream", index=False)
    return path, sorted_path


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (unsorted path, sorted path, fasta, the sorted file's table from the host reader, Sample.from_table of it): computed once."""
    d = str(tmp_path_factory.mktemp("unsorted"))
    out = {}
    for name, seed in (("collect_small", 11), ("ont_small", 12)):
        path, sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, name + ".bam"), d, seed)
        out[name] = (path, sorted_path, helpers.load_golden_fasta(name + ".fa.gz"))
    out["aligner"] = _htslike_files(d) + (bam.Fasta(sequences={"chrA": b"ACGT"}),)
    for name, (path, sorted_path, fasta) in list(out.items()):
        assert bam.read_bam_header(path).sort_order != "coordinate"
        want = bam.read_bam(sorted_path, with_seq=True)
        out[name] = (path, sorted_path, fasta, want, Sample.from_table(bam.read_bam(sorted_path, with_seq=True), fasta, MIN_SV, DEV))
    return out


def _check(sample, files, name, with_seq):
    _path, _sorted, _fasta, want, ref = files[name]
    sortcases.assert_same_table(sample.table, want, with_seq=with_seq, what=name)
    if not with_seq:
        assert sample.table.seq_packed is None
    assert np.array_equal(sample.gap_off, ref.gap_off) and np.array_equal(sample.stats, ref.stats)
    assert sample.gaps.dtype == ref.gaps.dtype and sample.gaps.tobytes() == ref.gaps.tobytes() and len(ref.gaps) > 0
    assert np.array_equal(sample.table.ref_span, ref.table.ref_span)


@pytest.mark.parametrize("ranges", ["one", "several"])
@pytest.mark.parametrize("name", ["collect_small", "ont_small", "aligner"])
def test_load_sample_equals_the_sorted_file(files, name, ranges):
    from svision_amd import ingest_sort
    path, _sorted, fasta = files[name][:3]
    stats = {}
    range_bytes = None if ranges == "one" else max(os.path.getsize(path) // 6, 1 << 16)
    sample = ingest_sort.load_sample(path, fasta, MIN_SV, device=DEV, with_seq=True, range_bytes=range_bytes, stats=stats)
    _check(sample, files, name, True)
    assert stats["records"] == len(files[name][3]) and (stats["ranges"] == 1 if ranges == "one" else stats["ranges"] >= 4), stats
    assert set(stats["seconds"]) == set(ingest_sort.STAGES)
    if name == "ont_small":
        assert int(np.diff(sample.table.cig_off).max()) == 3413
    if name == "aligner":
        assert int(np.diff(sample.table.cig_off).max()) > 65535 and int((sample.table.tid < 0).sum()) == 9 and (sample.table.tid[-9:] == -1).all()


def test_without_bases_and_the_sorted_file_itself(files):
    """with_seq=False carries no bases; a file that is sorted already goes through with the identity order: the same table."""
    from svision_amd import ingest_sort
    path, sorted_path, fasta = files["collect_small"][:3]
    _check(ingest_sort.load_sample(path, fasta, MIN_SV, device=DEV), files, "collect_small", False)
    for name in ("collect_small", "aligner"):
        _path, sorted_path, fasta = files[name][:3]
        _check(ingest_sort.load_sample(sorted_path, fasta, MIN_SV, device=DEV, with_seq=True), files, name, True)


def test_a_flipped_payload_byte_is_refused(files, tmp_path):
    from svision_amd import ingest_sort
    path, _sorted, fasta = files["collect_small"][:3]
    raw = bytearray(open(path, "rb").read())
    blocks = baicases.bgzf_blocks(bytes(raw))
    at = blocks[len(blocks) // 2][0] + 18 + 40                  # inside the DEFLATE payload of a block in the middle of the file
    raw[at] ^= 0x55
    bad = str(tmp_path / "flipped.bam")
    with open(bad, "wb") as f:
        f.write(bytes(raw))
    with pytest.raises(ingest_sort.SortIngestError, match="BGZF"):
        ingest_sort.load_sample(bad, fasta, MIN_SV, device=DEV)
    assert issubclass(ingest_sort.SortIngestError, ValueError)


# ---- the command line -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from oracle import alexnet_ref
    from svision_amd.network import tf_checkpoint as ck
    prefix = str(tmp_path_factory.mktemp("ckpt") / "svision-cnn-model.ckpt")
    ck.write_checkpoint(prefix, alexnet_ref.random_params(seed=7))
    return prefix


def _cli(args, env):
    base = {k: v for k, v in os.environ.items() if k not in ("SVX_DEVICE_SORT", "SVX_BUILD_INDEX", "SVX_INGEST")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "SVision")] + list(args), capture_output=True, text=True, timeout=900,
                          env=dict(base, PYTHONPATH=ROOT, SVX_TIMING="1", **env))


def _outputs(out, sample_name):
    seg = os.path.join(out, "segments")
    files = {f: open(os.path.join(seg, f), "rb").read() for f in sorted(os.listdir(seg))}
    vcf = os.path.join(out, "%s.svision.s3.vcf" % sample_name)
    return open(vcf, "rb").read() if os.path.exists(vcf) else None, files


def _genome(tmp_path, name):
    fasta = helpers.load_golden_fasta(name + ".fa.gz")
    fa = str(tmp_path / (name + ".fa"))
    bam.write_fasta(fa, {n: fasta._seq[n] for n in fasta.references})
    return fa


def test_command_line_on_a_shuffled_file(checkpoint, tmp_path):
    """SVX_DEVICE_SORT=1 on the shuffled collect_small, -t 1 and -t 3: the VCF and segments/ of the run on the stably sorted, indexed
    file, byte for byte.  Without the switch the file is refused as before; with it and two ranks it is refused too."""
    path, sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), tmp_path, 21)
    fa = _genome(tmp_path, "collect_small")
    args = ["-m", checkpoint, "-g", fa, "-n", "HGs", "-s", "3", "--window_size", "150000", "--batch_size", "64", "--debug"]
    outs = {}
    for what, src, t, env in (("sorted", sorted_path, "1", {}), ("device_sort", path, "1", {"SVX_DEVICE_SORT": "1"}),
                              ("device_sort_t3", path, "3", {"SVX_DEVICE_SORT": "1"})):
        out = str(tmp_path / ("out_" + what))
        r = _cli(["-o", out, "-b", src, "-t", t] + args, env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs[what] = _outputs(out, "HGs")
        log = "".join(open(os.path.join(out, f)).read() for f in os.listdir(out) if f.endswith(".log"))
        assert ("1491 records sorted on the device" in log) == (what != "sorted")
    assert outs["sorted"][0].count(b"\n") > 20 and sum(len(v) for v in outs["sorted"][1].values()) > 1000
    assert outs["device_sort"] == outs["sorted"]
    assert outs["device_sort_t3"] == outs["sorted"]
    out = str(tmp_path / "out_refused")
    r = _cli(["-o", out, "-b", path, "-t", "1"] + args, {})
    log = "".join(open(os.path.join(out, f)).read() for f in os.listdir(out) if f.endswith(".log"))
    assert r.returncode == 1 and "This is not a coordinate sorted BAM file" in log and "SVX_DEVICE_SORT=1" in log
    assert not os.path.exists(os.path.join(out, "HGs.svision.s3.vcf"))
    out = str(tmp_path / "out_ranks")
    r = _cli(["-o", out, "-b", path] + args, {"SVX_DEVICE_SORT": "1", "RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1",
                                               "MASTER_PORT": "29519"})
    log = "".join(open(os.path.join(out, f)).read() for f in os.listdir(out) if f.endswith(".log"))
    assert r.returncode == 1 and "single-rank run only" in log


def test_command_line_hash_on_a_shuffled_file(checkpoint, tmp_path):
    """--hash reads the bases of the sorted sample: the same files as the run on the sorted, indexed hash_collect."""
    path, sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "hash_collect.bam"), tmp_path, 22)
    fa = _genome(tmp_path, "hash_collect")
    args = ["-m", checkpoint, "-g", fa, "-n", "HGs", "-s", "3", "--hash", "--batch_size", "64", "--debug", "-t", "1"]
    outs = {}
    for what, src, env in (("sorted", sorted_path, {}), ("device_sort", path, {"SVX_DEVICE_SORT": "1"})):
        out = str(tmp_path / ("out_" + what))
        r = _cli(["-o", out, "-b", src] + args, env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs[what] = _outputs(out, "HGs")
    assert outs["device_sort"] == outs["sorted"] and sum(len(v) for v in outs["sorted"][1].values()) > 1000
