"""The index of a BAM that has none, built on the device (-m gpu): svx_bam_find_starts (csrc/svx_bamindex.hip) against a Python
walk of the file, svision_amd.index.build_index against tests/htslike.write_bai of the walked records -- byte for byte --, the
device decoder on the built index against the host decoder, and the driver's SVX_BUILD_INDEX switch.

The oracle (tests/baicases.walk: zlib + struct) shares no code with svision_amd/io/bai.py or svision_amd/index.py."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from svision_amd import _lib, index, kernels
from svision_amd.io import bam
from tests import baicases, helpers, htslike

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_START = baicases.NO_START


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, walk).  Every file holds a few hundred records on chrA and chrB; chrEmpty has none.  None has a .bai."""
    d = tmp_path_factory.mktemp("bai_gpu")
    out = {}
    for name, recs, level, policy in (("flushed1", baicases.short_records(), 1, "htslib"), ("flushed9", baicases.short_records(seed=3), 9, "htslib"),
                                      ("straddling", baicases.short_records(seed=4), 1, "stream"), ("cg", baicases.short_records(seed=6, n=120, cg=True), 6, "htslib")):
        path = str(d / (name + ".bam"))
        htslike.write_bam(path, baicases.REFS, recs, level=level, policy=policy, index=False)
        out[name] = (path, baicases.walk(path))
    # the product's own writer (blocks cut every 0xFF00 bytes, QUAL 0xFF, no tags) on the straddling file's records
    path = str(d / "own_writer.bam")
    bam.write_bam(path, bam.read_bam(out["straddling"][0], with_seq=True), with_seq=True, level=1, index=False)
    out["own_writer"] = (path, baicases.walk(path))
    out["long"] = (str(d / "long.bam"),) + baicases.write_long(str(d / "long.bam"))
    out["decoy"] = (str(d / "decoy.bam"),) + baicases.write_decoy(str(d / "decoy.bam"))
    assert not any(os.path.exists(v[0] + ".bai") for v in out.values())
    return out


def find_starts(walked, n_ref=None, first_block=0, n_blocks=None, entry=None, stream=None):
    """svx_bam_find_starts over the blocks [first_block, first_block + n_blocks) of a walked file -- the inflated bytes are the
    walk's own (zlib), so nothing but the kernels under test runs -- -> (d_first as uint64, exit, status, d_raw, offsets)."""
    lib = _lib.load()
    dev = torch.device("cuda:0")
    nb = len(walked.coff) - first_block if n_blocks is None else n_blocks
    base = walked.dst[first_block]
    dst = np.asarray(walked.dst[first_block:first_block + nb + 1], np.uint64) - np.uint64(base)
    raw = np.frombuffer((stream or walked.stream)[base:base + int(dst[-1])], np.uint8)
    padded = np.zeros((raw.size + 15) // 16 * 16 + 16, np.uint8)
    padded[:raw.size] = raw
    d_raw, d_dst = torch.from_numpy(padded).to(dev), torch.from_numpy(dst.view(np.int64)).to(dev)
    lengths = [l for _n, l in walked.references][:n_ref]
    d_len = torch.from_numpy(np.asarray(lengths + [0], np.int32)).to(dev)
    d_first = torch.full((nb,), 7, dtype=torch.int64, device=dev)
    d_exit = torch.full((2,), 7, dtype=torch.int64, device=dev)
    d_ws = torch.empty(int(lib.svx_bam_find_starts_ws_bytes(nb)), dtype=torch.uint8, device=dev)
    entry = (walked.header_end if entry is None else entry) - base
    _lib.check(lib.svx_bam_find_starts(d_raw.data_ptr(), d_dst.data_ptr(), nb, entry, len(lengths), d_len.data_ptr(), d_first.data_ptr(), d_exit.data_ptr(),
                                       d_ws.data_ptr(), int(d_ws.numel()), kernels._stream_ptr(dev)), "svx_bam_find_starts")
    ex = d_exit.cpu().numpy().view(np.uint64)
    return d_first.cpu().numpy().view(np.uint64), int(ex[0]), int(ex[1]), d_raw, dst


def check_file(files, name, tmp_path):
    """The two things every case asks: d_first == the walk's per-block first starts, build_index == htslike's index of the walk."""
    path, walked = files[name][:2]
    first, ex, status, _raw, _dst = find_starts(walked)
    assert status == 0 and ex == len(walked.stream)
    assert first.tolist() == walked.first
    out = str(tmp_path / (name + ".bai"))
    stats = {}
    assert index.build_index(path, out, stats=stats) == out
    assert open(out, "rb").read() == baicases.expected_bai(tmp_path, walked)
    assert stats["ranges"] == 1 and stats["records"] == len(walked.records) and sorted(os.listdir(tmp_path)) == sorted(["expected.bai", name + ".bai"])
    return walked


@pytest.mark.parametrize("name", ["flushed1", "flushed9"])
def test_flushed_blocks(files, name, tmp_path):
    """htslib's policy: a record that would not fit starts a fresh block -- every block's first start is its first byte.  Placed
    unmapped reads (flag 4 with a reference) and a tail of reads without one (n_no_coor)."""
    w = check_file(files, name, tmp_path)
    assert all(f == d for f, d in zip(w.first[1:-1], w.dst[1:-1])) and len(w.first) > 12
    assert sum(r["tid"] < 0 for r in w.records) == 9 and any(r["flag"] & 4 and r["tid"] >= 0 for r in w.records)
    assert open(str(tmp_path / (name + ".bai")), "rb").read()[-8:] == struct.pack("<Q", 9)


@pytest.mark.parametrize("name", ["straddling", "own_writer"])
def test_straddling_blocks(files, name, tmp_path):
    """Blocks cut every 0xFF00 bytes: every block's first start lies mid-block.  One file is svision_amd.io.bam.write_bam's."""
    w = check_file(files, name, tmp_path)
    inner = [(f, d) for f, d in zip(w.first[1:-1], w.dst[1:-1]) if f != NO_START]
    assert len(inner) >= 12 and all(f > d for f, d in inner)


def test_records_longer_than_a_block(files, tmp_path):
    """Reads of 100-200 kb: blocks without a start, a record over three blocks and more, a block_size field across a boundary."""
    w = check_file(files, "long", tmp_path)
    k = files["long"][2]
    assert w.offsets[k] % baicases.BLOCK == baicases.BLOCK - 2          # two bytes of the field end a block, two open the next
    assert w.first.count(NO_START) > 20
    assert max(w.block_of(b - 1) - w.block_of(a) for a, b in zip(w.offsets, w.offsets[1:])) >= 2


def test_a_decoy_is_picked_and_discarded(files, tmp_path):
    """A B,C array holds the exact bytes of two records and begins on the first byte of a block: the block's guess is the copy,
    the chain from the header's end arrives behind it, and the result is the true chain."""
    w = files["decoy"][1]
    at = files["decoy"][2]
    b = at // baicases.BLOCK
    assert at % baicases.BLOCK == 0 and at == w.dst[b] and at not in w.offsets and w.stream[at:at + len(baicases.decoy_copy())] == baicases.decoy_copy()
    assert w.first[b] not in (NO_START, at)                     # the block has a true start, and it is not the copy
    check_file(files, "decoy", tmp_path)


def test_every_guess_wrong_still_ends(files):
    """With an empty reference dictionary no header of a placed record is plausible: no block has a candidate, every link is
    broken, and the one resolving lane walks the whole file -- to the same answer."""
    w = files["straddling"][1]
    first, ex, status, _raw, _dst = find_starts(w, n_ref=0)
    assert status == 0 and ex == len(w.stream) and first.tolist() == w.first


@pytest.mark.parametrize("name", ["straddling", "long"])
def test_range_carry(files, name, tmp_path):
    """Ranges of 256 KB: records cut by range ends are carried into the next range (on the long reads: ranges in which no record
    completes are enlarged); the bytes are the one-range result's."""
    path, w = files[name][:2]
    one, many = str(tmp_path / "one.bai"), str(tmp_path / "many.bai")
    index.build_index(path, one)
    stats = {}
    index.build_index(path, many, range_bytes=256 << 10, stats=stats)
    assert stats["ranges"] >= 3 and stats["records"] == len(w.records)
    assert open(many, "rb").read() == open(one, "rb").read() == baicases.expected_bai(tmp_path, w)
    # a range in the middle of the file by hand: the exit is the start of the record its end cuts
    b0 = 2 if name == "straddling" else next(b for b in range(3, len(w.first)) if w.first[b] != NO_START)
    nb = 4 if name == "straddling" else 9
    first, ex, status, _raw, dst = find_starts(w, first_block=b0, n_blocks=nb, entry=w.first[b0])
    base, end = w.dst[b0], w.dst[b0 + nb]
    inside = [o for o in w.offsets if w.first[b0] <= o < end]
    cut = next(o for o, nxt in zip(w.offsets, w.offsets[1:] + [len(w.stream)]) if o >= w.first[b0] and nxt > end)
    assert status == 0 and ex == cut - base and cut < end
    want = [NO_START] * nb
    for o in reversed(inside):
        want[w.block_of(o) - b0] = o - base
    assert first.tolist() == want


def test_cg_tag_record(files, tmp_path):
    """An alignment of more than 65,535 operations: its bin and its linear-index windows come from the CIGAR in its CG tag."""
    w = check_file(files, "cg", tmp_path)
    cg = [r for r in w.records if len(r["cigar"]) > 65535]
    assert len(cg) == 1 and htslike.ref_len(cg[0]["cigar"]) == 33_540
    assert htslike.reg2bin(cg[0]["pos"], cg[0]["pos"] + 33_540) != htslike.reg2bin(cg[0]["pos"], cg[0]["pos"] + 1)


def _refused(path, tmp_path, match):
    out = str(tmp_path / "refused.bai")
    with pytest.raises(index.IndexBuildError, match=match):
        index.build_index(path, out)
    assert os.listdir(os.path.dirname(out)) == [os.path.basename(path)]


def test_refusals(files, tmp_path):
    """Malformed inputs the bounds checks catch; each raises and leaves no file."""
    w = files["straddling"][1]
    raw = open(files["straddling"][0], "rb").read()
    # cut inside a record: the file's last five data blocks dropped, the EOF block re-appended (the inflate itself succeeds)
    keep = len(w.coff) - 6
    assert w.dst[keep] not in w.offsets
    d = tmp_path / "cut"
    d.mkdir()
    with open(str(d / "cut.bam"), "wb") as f:
        f.write(raw[:w.coff[keep]] + htslike.EOF_BLOCK)
    _refused(str(d / "cut.bam"), d, "cut inside a record")
    # a block_size of 7
    d = tmp_path / "bs7"
    d.mkdir()
    s = bytearray(w.stream)
    s[w.offsets[150]:w.offsets[150] + 4] = struct.pack("<i", 7)
    baicases.write_stream(str(d / "bs7.bam"), bytes(s))
    first, ex, status, _raw, _dst = find_starts(w, stream=bytes(s))
    assert (ex, status) == (w.offsets[150], 1)
    _refused(str(d / "bs7.bam"), d, "malformed record")
    # two records swapped out of order
    d = tmp_path / "swapped"
    d.mkdir()
    recs = baicases.short_records(seed=4)
    assert (recs[40]["tid"], recs[40]["pos"]) < (recs[41]["tid"], recs[41]["pos"])
    recs[40], recs[41] = recs[41], recs[40]
    htslike.write_bam(str(d / "swapped.bam"), baicases.REFS, recs, level=1, policy="stream", index=False)
    _refused(str(d / "swapped.bam"), d, "not coordinate-sorted")


def _same_records(device_table, host_table):
    for f in ("tid", "pos", "flag", "mapq", "l_seq"):
        assert np.array_equal(getattr(device_table, f), getattr(host_table, f)), f
    assert np.array_equal(np.asarray(device_table.cigar), host_table.cigar) and np.array_equal(device_table.cig_off, host_table.cig_off)
    assert [device_table.names[i] for i in device_table.name_id] == [host_table.names[i] for i in host_table.name_id]


@pytest.mark.parametrize("name", ["flushed1", "straddling", "long"])
def test_the_walk_and_the_device_decoder_take_the_starts(files, name, tmp_path):
    """svx_bam_walk_count over the compacted d_first reports status 0 for every start, and DeviceDecoder on the built index
    returns, reference by reference, the host decoder's tables."""
    import svision_amd.ingest_gpu as ig
    path, w = files[name][:2]
    lib = _lib.load()
    first, ex, _status, d_raw, _dst = find_starts(w)
    starts = np.append(first[first != np.uint64(NO_START)], np.uint64(ex))
    d_starts = torch.from_numpy(starts.view(np.int64)).cuda()
    d_counts = torch.empty((starts.size - 1, 4), dtype=torch.int64, device="cuda:0")
    _lib.check(lib.svx_bam_walk_count(d_raw.data_ptr(), d_starts.data_ptr(), starts.size - 1, d_counts.data_ptr(), kernels._stream_ptr(torch.device("cuda:0"))),
               "svx_bam_walk_count")
    counts = d_counts.cpu().numpy()
    assert not counts[:, 3].any() and int(counts[:, 0].sum()) == len(w.records)
    built = index.build_index(path, str(tmp_path / "built.bai"))
    head = bam.read_bam_header(path)
    whole = bam.read_bam(path)                                  # the host decoder, without any index
    dec = ig.DeviceDecoder(path, built, head.references, head.lengths, head.header_text, "cuda:0", threads=3)
    assert dec.usable([0, 1, 2])
    seen = []
    for finish, _arrays in dec.parts_pipelined([0, 1, 2]):
        tb = finish()
        ig.spill_cigar(tb)
        t = int(tb.tid[0])
        seen.append(t)
        _same_records(tb, whole.subset(np.flatnonzero(whole.tid == t)))
    assert seen == [0, 2]


def test_driver_builds_the_index_when_asked(tmp_path):
    """SVX_BUILD_INDEX=1 and no .bai next to the BAM: the command line writes OUT/<name>.bai, runs on the device engine and
    writes the VCF of the run with the shipped index; without the variable the run is today's -- host engine, same VCF."""
    from oracle import alexnet_ref
    from svision_amd.network import tf_checkpoint as ck
    prefix = str(tmp_path / "m.ckpt")
    ck.write_checkpoint(prefix, alexnet_ref.random_params(seed=7))
    fasta = helpers.load_golden_fasta("collect_small.fa.gz")
    fa = str(tmp_path / "collect_small.fa")
    bam.write_fasta(fa, {n: fasta._seq[n] for n in fasta.references})
    shipped = str(tmp_path / "collect_small.bam")
    bam.write_bam(shipped, bam.read_bam(os.path.join(helpers.GOLDEN, "collect_small.bam")), index=True)
    os.mkdir(str(tmp_path / "bare"))
    bare = str(tmp_path / "bare" / "collect_small.bam")
    shutil.copy(shipped, bare)
    outs = {}
    for what, path, env in (("shipped", shipped, {}), ("built", bare, {"SVX_BUILD_INDEX": "1"}), ("bare", bare, {})):
        out = str(tmp_path / ("out_" + what))
        e = {k: v for k, v in os.environ.items() if k not in ("SVX_BUILD_INDEX", "SVX_INGEST")}
        r = subprocess.run([sys.executable, os.path.join(ROOT, "SVision"), "-o", out, "-b", path, "-m", prefix, "-g", fa, "-n", "HGi", "-s", "3",
                            "--window_size", "150000", "--batch_size", "64", "-t", "1"], capture_output=True, text=True, timeout=600,
                           env=dict(e, PYTHONPATH=ROOT, SVX_TIMING="1", **env))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert ("'engine': '%s'" % ("cpu" if what == "bare" else "gpu")) in r.stdout
        assert os.path.exists(os.path.join(out, "collect_small.bam.bai")) == (what == "built")
        outs[what] = open(os.path.join(out, "HGi.svision.s3.vcf")).read()
    assert os.listdir(str(tmp_path / "bare")) == ["collect_small.bam"]          # nothing is written next to the BAM
    assert outs["built"] == outs["shipped"] == outs["bare"] and outs["shipped"].count("\n") > 20
    # more than one rank: refused, with the command that builds the index first
    r = subprocess.run([sys.executable, os.path.join(ROOT, "SVision"), "-o", str(tmp_path / "out_ranks"), "-b", bare, "-m", prefix, "-g", fa, "-n", "HGi"],
                       capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT, SVX_BUILD_INDEX="1", RANK="0", WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29517"))
    assert r.returncode != 0
    log = "".join(open(os.path.join(str(tmp_path / "out_ranks"), f)).read() for f in os.listdir(str(tmp_path / "out_ranks")) if f.endswith(".log"))
    assert "python -m svision_amd.index" in log + r.stderr + r.stdout
