"""The ``.csi`` of a BAM that has no index, built on the device (-m gpu): svision_amd.index.build_index(fmt="csi") against
tests/csilike.py's index of the walked records -- the inflated bytes, byte for byte --, a 700 Mb reference with records on both sides
of 2^29 (which a ``.bai`` refuses), and the two command lines.  The first run of the index pass -- find-starts, the record walk,
svx_cigar_scan -- on positions from 2^29 on."""
import os
import shutil
import subprocess
import sys

import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from svision_amd import index
from svision_amd.io import bam, csi
from tests import baicases, csilike, helpers, htslike

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = 1 << 29


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, walk): three files of tests/baicases.py and the long-reference records, none with an index."""
    d = tmp_path_factory.mktemp("csi_gpu")
    out = {}
    for name, refs, recs, policy in (("flushed", baicases.REFS, baicases.short_records(), "htslib"), ("straddling", baicases.REFS, baicases.short_records(seed=4), "stream"),
                                     ("cg", baicases.REFS, baicases.short_records(seed=6, n=120, cg=True), "htslib"),
                                     ("long", csilike.LONG_REFS, csilike.long_records(), "htslib")):
        path = str(d / (name + ".bam"))
        htslike.write_bam(path, refs, recs, level=1, policy=policy, index=False)
        out[name] = (path, baicases.walk(path))
    return out


@pytest.mark.parametrize("name", ["flushed", "straddling", "cg"])
def test_build_equals_csilike(files, name, tmp_path):
    path, w = files[name]
    out = str(tmp_path / (name + ".csi"))
    stats = {}
    assert index.build_index(path, out, fmt="csi", stats=stats) == out
    data = open(out, "rb").read()
    assert csilike.inflate(data) == csilike.payload(w.references, w.records, w.voffs) and data.endswith(csilike.EOF_BLOCK)
    got = csi.read_csi(out)
    assert (got.min_shift, got.depth) == (14, 2) and got.n_no_coor == sum(r["tid"] < 0 for r in w.records)
    assert stats["records"] == len(w.records) and os.listdir(tmp_path) == [name + ".csi"]
    # smaller bins: one level more over the same references
    small = index.build_index(path, str(tmp_path / "m12.csi"), fmt="csi", min_shift=12)
    assert csilike.inflate(open(small, "rb").read()) == csilike.payload(w.references, w.records, w.voffs, min_shift=12)
    assert csi.read_csi(small).depth == 3
    # the default name, and the .bai of the same pass is unchanged
    d = tmp_path / "beside"
    d.mkdir()
    shutil.copy(path, str(d / "x.bam"))
    assert index.build_index(str(d / "x.bam"), fmt="csi") == str(d / "x.bam.csi") and index.build_index(str(d / "x.bam")) == str(d / "x.bam.bai")
    assert open(str(d / "x.bam.bai"), "rb").read() == baicases.expected_bai(tmp_path, w)
    with pytest.raises(ValueError, match="fmt"):
        index.build_index(path, out, fmt="tbi")


def test_long_reference(files, tmp_path):
    """Records up to 699,994,999 of a 700 Mb reference: fmt="bai" refuses by the first record that reaches 2^29 and leaves nothing,
    fmt="csi" gives depth 6 and an index through which every region reaches the records that overlap it."""
    path, w = files["long"]
    assert [r["pos"] for r in w.records] == [r["pos"] for r in csilike.long_records()] and max(r["pos"] for r in w.records) > 699_990_000
    first = next(r for r in w.records if r["tid"] == 0 and csilike.span_of(r)[1] - 1 >= EDGE)
    d = tmp_path / "refused"
    d.mkdir()
    with pytest.raises(index.IndexBuildError) as exc:
        index.build_index(path, str(d / "long.bam.bai"), fmt="bai")
    text = str(exc.value)
    assert "position %d of long" % first["pos"] in text and "a .bai cannot hold positions from 2^29 on" in text and "--csi" in text and "SVX_BUILD_INDEX=csi" in text
    with pytest.raises(index.IndexBuildError, match="cannot hold positions"):
        index.build_index(path, str(d / "default.bai"))
    assert os.listdir(d) == []
    out = index.build_index(path, str(tmp_path / "long.csi"), fmt="csi")
    assert csilike.inflate(open(out, "rb").read()) == csilike.payload(w.references, w.records, w.voffs)
    got = csi.read_csi(out)
    assert got.depth == 6 and got.meta[0][2:] == (sum(r["tid"] == 0 and not r["flag"] & 4 for r in w.records), 1)
    assert csilike.regions_match(csilike.as_idx(got), w.references, w.records, w.voffs, 500, seed=9) == 500
    # the host reader takes the reference's byte range from it
    whole = bam.read_bam(path)
    for t in (0, 1):
        part = bam.read_bam(path, tids=[t], index=out)
        assert part.pos.tolist() == whole.pos[whole.tid == t].tolist() and len(part) > 50


def test_command_line(files, tmp_path):
    """``python -m svision_amd.index --csi [-m N] [-o OUT]`` in a child process: BAM + .csi by default; without --csi the long
    reference is refused with status 1 and the switch in the message."""
    src, w = files["long"]
    path = str(tmp_path / "long.bam")
    shutil.copy(src, path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "svision_amd.index", path], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 1 and "--csi" in r.stderr and "position" in r.stderr and os.listdir(tmp_path) == ["long.bam"], r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-m", "svision_amd.index", "--csi", path], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and (path + ".csi") in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    assert csilike.inflate(open(path + ".csi", "rb").read()) == csilike.payload(w.references, w.records, w.voffs)
    r = subprocess.run([sys.executable, "-m", "svision_amd.index", "-c", "-m", "12", "-o", str(tmp_path / "m12.csi"), path], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert csilike.inflate(open(str(tmp_path / "m12.csi"), "rb").read()) == csilike.payload(w.references, w.records, w.voffs, min_shift=12)
    assert sorted(os.listdir(tmp_path)) == ["long.bam", "long.bam.csi", "m12.csi"]


def test_driver_builds_a_csi_when_asked(tmp_path):
    """SVX_BUILD_INDEX=csi and no index next to the BAM: the command line writes OUT/<name>.bam.csi and the device engine runs from it."""
    from oracle import alexnet_ref
    from svision_amd.network import tf_checkpoint as ck
    prefix = str(tmp_path / "m.ckpt")
    ck.write_checkpoint(prefix, alexnet_ref.random_params(seed=7))
    fasta = helpers.load_golden_fasta("collect_small.fa.gz")
    fa = str(tmp_path / "collect_small.fa")
    bam.write_fasta(fa, {n: fasta._seq[n] for n in fasta.references})
    os.mkdir(str(tmp_path / "bare"))
    bare = str(tmp_path / "bare" / "collect_small.bam")
    bam.write_bam(bare, bam.read_bam(os.path.join(helpers.GOLDEN, "collect_small.bam")), index=False)
    out = str(tmp_path / "out")
    e = {k: v for k, v in os.environ.items() if k not in ("SVX_BUILD_INDEX", "SVX_INGEST")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "SVision"), "-o", out, "-b", bare, "-m", prefix, "-g", fa, "-n", "HGi", "-s", "3",
                        "--window_size", "150000", "--batch_size", "64", "-t", "1"], capture_output=True, text=True, timeout=600,
                       env=dict(e, PYTHONPATH=ROOT, SVX_TIMING="1", SVX_BUILD_INDEX="csi"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "'engine': 'gpu'" in r.stdout
    built = os.path.join(out, "collect_small.bam.csi")
    assert os.path.exists(built) and not os.path.exists(os.path.join(out, "collect_small.bam.bai")) and os.listdir(str(tmp_path / "bare")) == ["collect_small.bam"]
    w = baicases.walk(bare)
    assert csilike.inflate(open(built, "rb").read()) == csilike.payload(w.references, w.records, w.voffs)
    assert open(os.path.join(out, "HGi.svision.s3.vcf")).read().count("\n") > 20
    log = "".join(open(os.path.join(out, f)).read() for f in os.listdir(out) if f.endswith(".log"))
    assert "device engine" in log and "collect_small.bam.csi" in log
