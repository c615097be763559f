"""The device-sorted BAM as a file (svision_amd/sort.py, SVX_DEVICE_SORT=write): sort_bam on the three unsorted files of
tests/test_gpu_unsorted_bam.py -- record-shuffled golden files and a file of the test-side writer (no @HD line, records across BGZF
blocks, a CG-tag CIGAR, records without a reference in the middle).  The written file is taken apart with zlib and struct
(tests/baicases.walk), its records compared byte for byte with the input's in tests/sortcases.order, its .bai with the
htslike-convention index of the walked file; the host reader and the device decoder read it; small and default chunking agree; broken
inputs leave nothing behind; and the command line calls the same variants from it as SVX_DEVICE_SORT=1 and the pre-sorted file."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from svision_amd.io import bam
from tests import baicases, helpers, htslike, sortcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _raw_records(w):
    """The walked file's records as bytes, in file order."""
    ends = w.offsets[1:] + [len(w.stream)]
    return [w.stream[a:b] for a, b in zip(w.offsets, ends)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> dict: the unsorted path, the reference sorted path, the input walked, and sort_bam's outputs with small ranges and chunks
    ("small") and with the defaults ("default") as (path, stats): computed once."""
    from svision_amd import sort
    d = str(tmp_path_factory.mktemp("sort_write"))
    out = {}
    for name, seed in (("collect_small", 11), ("ont_small", 12)):
        path, sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, name + ".bam"), d, seed)
        out[name] = dict(path=path, sorted=sorted_path)
    path, sorted_path = _htslike_files(d)
    out["aligner"] = dict(path=path, sorted=sorted_path)
    for name, f in out.items():
        assert bam.read_bam_header(f["path"]).sort_order != "coordinate"
        f["walked"] = w = baicases.walk(f["path"])
        # >= 4 ranges of the pass (compressed bytes), >= 3 chunks of the output (inflated bytes, whole blocks)
        range_bytes = max(os.path.getsize(f["path"]) // 6, 1 << 16)
        chunk_bytes = max((len(w.stream) - w.header_end) // 4 // htslike.BLOCK, 1) * htslike.BLOCK
        for what, kw in (("small", dict(range_bytes=range_bytes, chunk_bytes=chunk_bytes)), ("default", {})):
            stats = {}
            p = os.path.join(d, "%s.%s.out.bam" % (name, what))
            assert sort.sort_bam(f["path"], p, device=DEV, stats=stats, **kw) == p
            f[what] = (p, stats)
    return out


@pytest.mark.parametrize("name", ["collect_small", "ont_small", "aligner"])
def test_the_written_file(files, name, tmp_path):
    from svision_amd import sort
    f = files[name]
    out, stats = f["small"]
    assert stats["ranges"] >= 4 and stats["chunks"] >= 3 and set(stats["seconds"]) == set(sort.STAGES), stats
    raw = open(out, "rb").read()
    assert raw.endswith(htslike.EOF_BLOCK)
    w_in, w_out = f["walked"], baicases.walk(out)
    # gzip reads the whole file: header + records
    assert gzip.decompress(raw) == w_out.stream
    text = w_out.stream[8:8 + int.from_bytes(w_out.stream[4:8], "little")].decode()
    assert text.split("\n")[0].split("\t")[:3] == ["@HD", "VN:1.6", "SO:coordinate"] and "@PG\tID:svision" not in text
    assert text.split("\n")[1:] == [l for l in w_in.stream[8:8 + int.from_bytes(w_in.stream[4:8], "little")].decode().split("\n") if not l.startswith("@HD")]
    assert w_out.references == w_in.references
    # the record region: the input's raw records, byte for byte, in sortcases.order
    recs = _raw_records(w_in)
    o = sortcases.order(np.asarray([r["tid"] for r in w_in.records]), np.asarray([r["pos"] for r in w_in.records]), len(w_in.references))
    want = b"".join(recs[i] for i in o)
    assert w_out.stream[w_out.header_end:] == want
    assert stats["records"] == len(recs) and stats["inflated_bytes"] == len(w_out.stream) and stats["compressed_bytes"] == len(raw)
    assert stats["blocks"] == len(w_out.coff)
    # the header has blocks of its own, records are cut every 0xFF00 bytes of their stream
    sizes = np.diff(w_out.dst).tolist()
    n_head = -(-w_out.header_end // htslike.BLOCK)
    assert w_out.dst[n_head] == w_out.header_end and sizes[-1] == 0
    assert all(s == htslike.BLOCK for s in sizes[n_head:-2]) and 0 < sizes[-2] <= htslike.BLOCK
    if name == "aligner":
        ref = baicases.walk(f["sorted"])
        assert w_out.stream[w_out.header_end:] == ref.stream[ref.header_end:]
        tids = [r["tid"] for r in w_out.records]
        assert tids[-9:] == [-1] * 9 and -1 not in tids[:-9] and max(len(r["cigar"]) for r in w_out.records) > 65535
    # the index: htslike's of the walked output, byte for byte
    assert open(out + ".bai", "rb").read() == baicases.expected_bai(tmp_path, w_out)
    # small and default chunking: the same files
    assert open(f["default"][0], "rb").read() == raw
    assert open(f["default"][0] + ".bai", "rb").read() == open(out + ".bai", "rb").read()
    assert f["default"][1]["ranges"] == 1 and f["default"][1]["chunks"] == 1
    assert not [n for n in os.listdir(os.path.dirname(out)) if n.endswith(".tmp")]


@pytest.mark.parametrize("name", ["collect_small", "ont_small", "aligner"])
def test_the_readers_accept_it(files, name):
    """The host reader gives the table of the reference sorted file; the device decoder on the file and its index equals the host's."""
    from svision_amd import ingest_gpu
    f = files[name]
    out = f["small"][0]
    got, want = bam.read_bam(out, with_seq=True), bam.read_bam(f["sorted"], with_seq=True)
    sortcases.assert_same_table(got, want, with_seq=True, what=name)
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
            assert np.array_equal(getattr(tb, fld), getattr(host, fld)), (name, t, fld)
        assert np.array_equal(np.asarray(tb.cigar), host.cigar) and np.array_equal(tb.cig_off, host.cig_off)
        assert [tb.names[i] for i in tb.name_id] == [host.names[i] for i in host.name_id]
    assert seen == sorted(set(int(t) for t in whole.tid if t >= 0))


def test_broken_inputs_leave_nothing(files, tmp_path):
    from svision_amd import sort
    path = files["collect_small"]["path"]
    raw = open(path, "rb").read()
    cut = str(tmp_path / "cut.bam")
    with open(cut, "wb") as f:
        f.write(raw[:len(raw) * 2 // 3])
    flipped = bytearray(raw)
    blocks = baicases.bgzf_blocks(raw)
    flipped[blocks[len(blocks) // 2][0] + 18 + 40] ^= 0x55          # inside the DEFLATE payload of a block in the middle of the file
    flip = str(tmp_path / "flipped.bam")
    with open(flip, "wb") as f:
        f.write(bytes(flipped))
    before = sorted(os.listdir(str(tmp_path)))
    for bad in (cut, flip):
        with pytest.raises(sort.SortWriteError):
            sort.sort_bam(bad, str(tmp_path / "never.bam"), device=DEV, range_bytes=1 << 16, chunk_bytes=1 << 16)
        assert sorted(os.listdir(str(tmp_path))) == before
    with pytest.raises(sort.SortWriteError):
        sort.sort_bam(path, str(tmp_path / "no_such_dir" / "out.bam"), device=DEV)


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


def test_command_line_writes_and_calls_from_the_sorted_file(checkpoint, tmp_path):
    """SVX_DEVICE_SORT=write on the shuffled collect_small: the VCF and segments/ of SVX_DEVICE_SORT=1 and of the run on the
    pre-sorted, indexed file, byte for byte; the sorted file and its index stay in the output directory, and a plain run on them
    gives the same VCF.  Two ranks are refused with the module's name."""
    path, sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), tmp_path, 21)
    fasta = helpers.load_golden_fasta("collect_small.fa.gz")
    fa = str(tmp_path / "collect_small.fa")
    bam.write_fasta(fa, {n: fasta._seq[n] for n in fasta.references})
    args = ["-m", checkpoint, "-g", fa, "-n", "HGs", "-s", "3", "--window_size", "150000", "--batch_size", "64", "--debug", "-t", "1"]
    outs = {}
    written = os.path.join(str(tmp_path / "out_write"), "collect_small.shuffled.sorted.bam")
    for what, src, env in (("sorted", sorted_path, {}), ("device_sort", path, {"SVX_DEVICE_SORT": "1"}), ("write", path, {"SVX_DEVICE_SORT": "write"}),
                           ("again", written, {})):
        out = str(tmp_path / ("out_" + what))
        r = _cli(["-o", out, "-b", src] + args, env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs[what] = _outputs(out, "HGs")
        log = "".join(open(os.path.join(out, f)).read() for f in os.listdir(out) if f.endswith(".log"))
        assert ("1491 records sorted on the device" in log) == (what in ("device_sort", "write"))
        if what == "write":
            assert os.path.exists(written) and os.path.exists(written + ".bai") and "streamed from %s" % written in log
            assert not [n for n in os.listdir(out) if n.endswith(".tmp") or n.endswith(".json")]
    assert outs["sorted"][0].count(b"\n") > 20 and sum(len(v) for v in outs["sorted"][1].values()) > 1000
    assert outs["write"] == outs["sorted"] == outs["device_sort"]
    assert outs["again"][0] == outs["sorted"][0]
    out = str(tmp_path / "out_ranks")
    r = _cli(["-o", out, "-b", path] + args, {"SVX_DEVICE_SORT": "write", "RANK": "0", "WORLD_SIZE": "2", "LOCAL_RANK": "0", "MASTER_ADDR": "127.0.0.1",
                                               "MASTER_PORT": "29520"})
    log = "".join(open(os.path.join(out, f)).read() for f in os.listdir(out) if f.endswith(".log"))
    assert r.returncode == 1 and "python -m svision_amd.sort" in log and not os.path.exists(os.path.join(out, "collect_small.shuffled.sorted.bam"))
