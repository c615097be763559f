"""sort_bam with ``index_format="csi"`` (svision_amd/sort.py; -m gpu): the sorted file's bytes do not depend on the index format, the
``.csi`` beside it is tests/csilike.py's of the walked output, and records beyond 2^29 -- shuffled, as a BAM and as SAM text -- are
refused under the default ``.bai`` with nothing left and written with ``--csi``.  The first run of svx_record_sort at ``pos_bits`` 30,
of svx_sam_measure / svx_sam_encode and of the deflate road on such positions."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from svision_amd.io import bam, csi
from tests import baicases, csilike, helpers, htslike, samtext, sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = 1 << 29


def _raw_records(w):
    ends = w.offsets[1:] + [len(w.stream)]
    return [w.stream[a:b] for a, b in zip(w.offsets, ends)]


def _check_csi(path, w=None):
    """``path + ".csi"`` is csilike's index of the walked file, and through it every region reaches the records that overlap it."""
    w = w or baicases.walk(path)
    data = open(path + ".csi", "rb").read()
    assert csilike.inflate(data) == csilike.payload(w.references, w.records, w.voffs) and data.endswith(csilike.EOF_BLOCK)
    got = csi.read_csi(path + ".csi")
    assert csilike.regions_match(csilike.as_idx(got), w.references, w.records, w.voffs, 500, seed=13) == 500
    return w, got


def test_shuffled_golden_set(tmp_path):
    """collect_small, record-shuffled as in tests/test_gpu_sort_write.py: the .bam of the csi run is the default run's, byte for byte."""
    from svision_amd import sort
    path, _sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), str(tmp_path), 11)
    for name in ("d", "c"):
        os.mkdir(str(tmp_path / name))
    default, as_csi = str(tmp_path / "d" / "out.bam"), str(tmp_path / "c" / "out.bam")
    range_bytes = max(os.path.getsize(path) // 6, 1 << 16)
    stats = {}
    sort.sort_bam(path, default, device=DEV, range_bytes=range_bytes)
    assert sort.sort_bam(path, as_csi, device=DEV, range_bytes=range_bytes, index_format="csi", stats=stats) == as_csi
    assert open(as_csi, "rb").read() == open(default, "rb").read() and stats["ranges"] >= 4
    assert sorted(os.listdir(str(tmp_path / "c"))) == ["out.bam", "out.bam.csi"] and sorted(os.listdir(str(tmp_path / "d"))) == ["out.bam", "out.bam.bai"]
    w, got = _check_csi(as_csi)
    assert got.depth == csi.depth_for(max(l for _n, l in w.references)) and got.n_no_coor == sum(r["tid"] < 0 for r in w.records)
    # both indexes give the readers the same byte ranges
    assert csi.spans(as_csi + ".csi") == bam.read_bai(default + ".bai")
    for t in range(len(w.references)):
        a, b = bam.read_bam(as_csi, tids=[t], index=as_csi + ".csi"), bam.read_bam(default, tids=[t], index=default + ".bai")
        assert a.pos.tolist() == b.pos.tolist() and a.tid.tolist() == b.tid.tolist()
    with pytest.raises(ValueError, match="index_format"):
        sort.sort_bam(path, str(tmp_path / "x.bam"), device=DEV, index_format="tbi")


@pytest.fixture(scope="module")
def long_inputs(tmp_path_factory):
    """The long-reference records shuffled, as an unsorted BAM and as SAM text under the same header -> (bam, sam, records in input order)."""
    d = str(tmp_path_factory.mktemp("csi_sort"))
    recs = csilike.long_records()
    perm = np.random.default_rng(21).permutation(len(recs))
    shuffled = [recs[i] for i in perm]
    text = samtext.header_text(csilike.LONG_REFS)
    bam_path, sam_path = os.path.join(d, "long.unsorted.bam"), os.path.join(d, "long.sam")
    htslike.write_bam(bam_path, csilike.LONG_REFS, [samtext.for_htslike(r) for r in shuffled], level=1, policy="stream", header_text=text, index=False)
    with open(sam_path, "wb") as f:
        f.write(samtext.text(csilike.LONG_REFS, shuffled, header=text))
    return bam_path, sam_path, shuffled


@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_long_reference_default_refuses(long_inputs, kind, tmp_path):
    from svision_amd import sort
    path = long_inputs[0 if kind == "bam" else 1]
    with pytest.raises(sort.SortWriteError) as exc:
        sort.sort_bam(path, str(tmp_path / "out.bam"), device=DEV)
    first = min(r["pos"] for r in long_inputs[2] if r["tid"] == 0 and csilike.span_of(r)[1] - 1 >= EDGE)
    text = str(exc.value)
    assert "position %d of long" % first in text and "a .bai cannot hold positions from 2^29 on" in text and "--csi" in text and "SVX_SORT_INDEX=csi" in text
    assert os.listdir(tmp_path) == []


def test_long_reference_with_csi(long_inputs, tmp_path):
    """The record region is the input's records in stable coordinate order; SAM text and BAM give the same two files."""
    from svision_amd import sort
    bam_path, sam_path, shuffled = long_inputs
    from_bam, from_sam, stats = str(tmp_path / "b.bam"), str(tmp_path / "s.bam"), {}
    sort.sort_bam(bam_path, from_bam, device=DEV, index_format="csi", stats=stats)
    assert stats["pos_bits"] == 30 and stats["records"] == len(shuffled)
    w_in, w_out = baicases.walk(bam_path), baicases.walk(from_bam)
    recs = _raw_records(w_in)
    o = sortcases.order(np.asarray([r["tid"] for r in shuffled]), np.asarray([r["pos"] for r in shuffled]), len(csilike.LONG_REFS))
    assert w_out.stream[w_out.header_end:] == b"".join(recs[i] for i in o)
    assert [r["pos"] for r in w_out.records] == [shuffled[i]["pos"] for i in o] and max(r["pos"] for r in w_out.records) > 699_990_000
    _w, got = _check_csi(from_bam, w_out)
    assert got.depth == 6
    stats = {}
    sort.sort_bam(sam_path, from_sam, device=DEV, index_format="csi", stats=stats)
    assert stats["input"] == "sam" and stats["host_lines"] == 0 and stats["pos_bits"] == 30        # (every line is the kernels')
    assert open(from_sam, "rb").read() == open(from_bam, "rb").read() and open(from_sam + ".csi", "rb").read() == open(from_bam + ".csi", "rb").read()
    assert sorted(os.listdir(tmp_path)) == ["b.bam", "b.bam.csi", "s.bam", "s.bam.csi"]
    # the host reader on the sorted file, whole and by reference through the .csi
    whole = bam.read_bam(from_bam)
    assert whole.pos.tolist() == [r["pos"] for r in w_out.records]
    assert bam.read_bam(from_bam, tids=[1], index=from_bam + ".csi").pos.tolist() == [r["pos"] for r in w_out.records if r["tid"] == 1]


def test_command_line_and_variable(long_inputs, tmp_path):
    """``python -m svision_amd.sort --csi`` and ``SVX_SORT_INDEX=csi`` in a child process; without either the long reference is refused."""
    bam_path = long_inputs[0]
    env = {k: v for k, v in os.environ.items() if k != "SVX_SORT_INDEX"}
    env["PYTHONPATH"] = ROOT
    outs = {}
    for what, flags, extra, status in (("refused", [], {}, 1), ("flag", ["--csi"], {}, 0), ("variable", [], {"SVX_SORT_INDEX": "csi"}, 0)):
        d = tmp_path / what
        d.mkdir()
        r = subprocess.run([sys.executable, "-m", "svision_amd.sort", bam_path, "-o", str(d / "out.bam")] + flags, capture_output=True, text=True, timeout=300,
                           env=dict(env, **extra))
        assert r.returncode == status, r.stdout[-1000:] + r.stderr[-3000:]
        if status:
            assert "--csi" in r.stderr and "2^29" in r.stderr and os.listdir(d) == []
        else:
            assert sorted(os.listdir(d)) == ["out.bam", "out.bam.csi"]
            outs[what] = (open(str(d / "out.bam"), "rb").read(), open(str(d / "out.bam.csi"), "rb").read())
    assert outs["flag"] == outs["variable"]
    r = subprocess.run([sys.executable, "-m", "svision_amd.sort", bam_path, "-o", str(tmp_path / "x.bam")], capture_output=True, text=True, timeout=120,
                       env=dict(env, SVX_SORT_INDEX="tbi"))
    assert r.returncode == 2 and "SVX_SORT_INDEX" in r.stderr
