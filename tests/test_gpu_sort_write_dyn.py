"""sort_bam(..., tables="dynamic") (svision_amd/sort.py over svx_bgzf_deflate_dyn) on the `aligner` file of
tests/test_gpu_sort_write.py -- the test-side writer's unsorted file: no @HD line, records across BGZF blocks, a CG-tag CIGAR, records
without a reference in the middle.  The written file inflates to the bytes of the tables="fixed" output and is smaller, ends in the
end-of-file marker, has dynamic blocks, carries the index of its own walked blocks, is read by the host reader and the device decoder
like the reference sorted file, is the same under small and default chunking, and is what `python -m svision_amd.sort --tables
dynamic` and SVX_SORT_TABLES=dynamic write."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from svision_amd.io import bam
from tests import baicases, htslike, sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _aligner_files(d):
    """tests/test_gpu_sort_write.py's _htslike_files: unsorted records under a header without @HD -> (path, sorted path)."""
    recs = baicases.short_records(seed=8, n=120, cg=True)
    perm = np.random.default_rng(8).permutation(len(recs))
    shuffled = [recs[i] for i in perm]
    tids = [r["tid"] for r in shuffled]
    text = "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in baicases.REFS) + "@PG\tID:aligner\tPN:aligner\n"
    path, sorted_path = os.path.join(d, "aligner.bam"), os.path.join(d, "aligner.sorted.bam")
    htslike.write_bam(path, baicases.REFS, shuffled, level=1, policy="stream", header_text=text, index=False)
    o = sortcases.order(np.asarray(tids), np.asarray([r["pos"] for r in shuffled]), len(baicases.REFS))
    htslike.write_bam(sorted_path, baicases.REFS, [shuffled[i] for i in o], level=1, policy="stream", index=False)
    return path, sorted_path


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """The unsorted path, the reference sorted path, and sort_bam's outputs as (path, stats): dynamic tables with small ranges and chunks
    ("small") and with the defaults ("default"), fixed tables with the defaults ("fixed")."""
    from svision_amd import sort
    d = str(tmp_path_factory.mktemp("sort_write_dyn"))
    path, sorted_path = _aligner_files(d)
    w = baicases.walk(path)
    range_bytes = max(os.path.getsize(path) // 6, 1 << 16)
    chunk_bytes = max((len(w.stream) - w.header_end) // 4 // htslike.BLOCK, 1) * htslike.BLOCK
    out = dict(dir=d, path=path, sorted=sorted_path)
    for what, kw in (("small", dict(tables="dynamic", range_bytes=range_bytes, chunk_bytes=chunk_bytes)), ("default", dict(tables="dynamic")),
                     ("fixed", dict(tables="fixed"))):
        stats = {}
        p = os.path.join(d, "aligner.%s.out.bam" % what)
        assert sort.sort_bam(path, p, device=DEV, stats=stats, **kw) == p
        out[what] = (p, stats)
    return out


def test_the_written_file(written, tmp_path):
    from svision_amd import sort
    out, stats = written["small"]
    fixed, fixed_stats = written["fixed"]
    assert stats["ranges"] >= 4 and stats["chunks"] >= 3 and set(stats["seconds"]) == set(sort.STAGES), stats
    raw, raw_fixed = open(out, "rb").read(), open(fixed, "rb").read()
    assert raw.endswith(htslike.EOF_BLOCK)
    # the same inflated bytes in a smaller file
    assert gzip.decompress(raw) == gzip.decompress(raw_fixed)
    assert len(raw) < len(raw_fixed) and stats["compressed_bytes"] == len(raw) and fixed_stats["compressed_bytes"] == len(raw_fixed)
    assert stats["dynamic_blocks"] > 0 and fixed_stats["dynamic_blocks"] == 0
    assert stats["blocks"] == fixed_stats["blocks"] and stats["inflated_bytes"] == fixed_stats["inflated_bytes"]
    w_out = baicases.walk(out)
    assert stats["blocks"] == len(w_out.coff) and stats["inflated_bytes"] == len(w_out.stream)
    kinds = [(raw[int(at) + 18] >> 1) & 3 for at in w_out.coff]
    assert kinds.count(2) == stats["dynamic_blocks"] and kinds.count(0) == stats["stored_blocks"] and kinds[-1] == 1
    # the index: htslike's of the walked output, byte for byte
    assert open(out + ".bai", "rb").read() == baicases.expected_bai(tmp_path, w_out)
    # small and default chunking: the same files
    assert open(written["default"][0], "rb").read() == raw
    assert open(written["default"][0] + ".bai", "rb").read() == open(out + ".bai", "rb").read()
    assert written["default"][1]["ranges"] == 1 and written["default"][1]["chunks"] == 1
    assert not [n for n in os.listdir(written["dir"]) if n.endswith(".tmp")]
    with pytest.raises(ValueError):
        sort.sort_bam(written["path"], str(tmp_path / "never.bam"), device=DEV, tables="static")
    assert not os.path.exists(str(tmp_path / "never.bam"))


def test_the_readers_accept_it(written):
    """The host reader gives the table of the reference sorted file; the device decoder on the file and its index equals the host's."""
    from svision_amd import ingest_gpu
    out = written["small"][0]
    got, want = bam.read_bam(out, with_seq=True), bam.read_bam(written["sorted"], with_seq=True)
    sortcases.assert_same_table(got, want, with_seq=True, what="aligner")
    assert got.sort_order == "coordinate"
    head = bam.read_bam_header(out)
    whole = bam.read_bam(out)                                   # the host decoder, without any index
    tids = list(range(len(head.references)))
    dec = ingest_gpu.DeviceDecoder(out, out + ".bai", head.references, head.lengths, head.header_text, DEV, threads=3)
    assert dec.usable(tids)
    seen = []
    for finish, _arrays in dec.parts_pipelined(tids):
        tb = finish()
        ingest_gpu.spill_cigar(tb)
        t = int(tb.tid[0])
        seen.append(t)
        host = whole.subset(np.flatnonzero(whole.tid == t))
        for fld in ("tid", "pos", "flag", "mapq", "l_seq"):
            assert np.array_equal(getattr(tb, fld), getattr(host, fld)), (t, fld)
        assert np.array_equal(np.asarray(tb.cigar), host.cigar) and np.array_equal(tb.cig_off, host.cig_off)
        assert [tb.names[i] for i in tb.name_id] == [host.names[i] for i in host.name_id]
    assert seen == sorted(set(int(t) for t in whole.tid if t >= 0))


def test_the_command_line_and_the_environment_variable(written, tmp_path):
    """One child process with --tables dynamic writes the file sort_bam wrote; a second one with SVX_SORT_TABLES=dynamic and no option
    would be the same code path behind argparse's default, which is checked here without a process."""
    from svision_amd import sort
    base = {k: v for k, v in os.environ.items() if k != "SVX_SORT_TABLES"}
    out = str(tmp_path / "cli.bam")
    r = subprocess.run([sys.executable, "-m", "svision_amd.sort", written["path"], "-o", out, "--tables", "dynamic", "--device", DEV, "--stats-json",
                        str(tmp_path / "stats.json")], capture_output=True, text=True, timeout=600, env=dict(base, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "dynamic" in r.stdout
    assert open(out, "rb").read() == open(written["default"][0], "rb").read()
    assert open(out + ".bai", "rb").read() == open(written["default"][0] + ".bai", "rb").read()
    # SVX_SORT_TABLES: the option's default
    seen = {}
    real = sort.sort_bam

    def spy(*a, **kw):
        seen.update(kw)
        kw["stats"].update(records=0, blocks=0, stored_blocks=0, dynamic_blocks=0, inflated_bytes=0, compressed_bytes=0, ranges=0, chunks=0, seconds={})
        return a[1]
    sort.sort_bam = spy
    old = os.environ.get("SVX_SORT_TABLES")
    try:
        for value, want in (("dynamic", "dynamic"), ("", "fixed"), (None, "fixed")):
            os.environ.pop("SVX_SORT_TABLES", None)
            if value is not None:
                os.environ["SVX_SORT_TABLES"] = value
            assert sort.main([written["path"], "-o", str(tmp_path / "x.bam")]) == 0 and seen["tables"] == want
        os.environ["SVX_SORT_TABLES"] = "dynamic"
        assert sort.main([written["path"], "-o", str(tmp_path / "x.bam"), "--tables", "fixed"]) == 0 and seen["tables"] == "fixed"
    finally:
        sort.sort_bam = real
        os.environ.pop("SVX_SORT_TABLES", None)
        if old is not None:
            os.environ["SVX_SORT_TABLES"] = old
