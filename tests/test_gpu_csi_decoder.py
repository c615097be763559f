"""The device ingest engine driven from a ``.csi`` (svision_amd/ingest_gpu.py over io.csi.CsiSpan; -m gpu): against the same engine
driven from the ``.bai`` of the same file -- table for table at three group sizes, in small slices, with read bases --, every slice
complete on the first plan, a 700 Mb reference with records and windows on both sides of 2^29 against the host reader (the first run
of the record walk and of svx_cigar_scan on such positions), and the command line with nothing but a ``.csi`` beside the BAM."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from svision_amd import _lib, index, ingest
from svision_amd.io import bam, csi
from tests import csilike, helpers, htslike

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
EDGE = 1 << 29
WINDOW = 30_000
GROUP_SIZES = ((1 << 10, 1 << 10), (64 << 10, 96 << 10), (1 << 40, 1 << 40))


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    """name -> dict(path: a copy of the golden file written with its .bai, csi / csi12: indexes built on the device in a directory of
    their own, fasta: the genome's sequences)."""
    d = tmp_path_factory.mktemp("csi_decoder")
    out = {}
    for name in ("collect_small", "ont_small"):
        path = str(d / (name + ".bam"))
        bam.write_bam(path, bam.read_bam(os.path.join(helpers.GOLDEN, name + ".bam"), with_seq=True), with_seq=True, index=True)
        os.mkdir(str(d / (name + "_idx")))
        out[name] = dict(path=path, bai=path + ".bai", csi=index.build_index(path, str(d / (name + "_idx") / "x.csi"), fmt="csi"),
                         csi12=index.build_index(path, str(d / (name + "_idx") / "x12.csi"), fmt="csi", min_shift=12),
                         fasta=helpers.load_golden_fasta(name + ".fa.gz"))
    return out


@pytest.fixture()
def group_sizes():
    import svision_amd.ingest_gpu as ig
    saved = ig.FIRST_GROUP_BYTES, ig.PIPE_GROUP_BYTES
    yield ig
    ig.FIRST_GROUP_BYTES, ig.PIPE_GROUP_BYTES = saved


def _same(a, b, what=None):
    for f in ("tid", "pos", "flag", "mapq", "l_seq", "cig_off"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (f, what)
    assert np.array_equal(np.asarray(a.cigar), np.asarray(b.cigar)), what
    assert [a.names[i] for i in a.name_id] == [b.names[i] for i in b.name_id], what


def _range_table(path, vlo, vhi):
    lib = _lib.load()
    h = lib.svx_bam_open_range(path.encode(), 2, 0, vlo, vhi)
    assert h, lib.svx_bam_error().decode()
    return bam._table_from_handle(lib, h, False)


def _decoder(ig, path, idx, with_seq=False):
    head = bam.read_bam_header(path)
    return ig.DeviceDecoder(path, idx, head.references, head.lengths, head.header_text, DEV, threads=3, with_seq=with_seq), head


def _whole_tables(ig, path, idx, with_seq=False):
    dec, head = _decoder(ig, path, idx, with_seq)
    tids = list(range(len(head.references)))
    assert dec.usable(tids)
    out = {}
    for finish, (_d_cigar, d_off, d_pos) in dec.parts_pipelined(tids):
        tb = finish()
        ig.spill_cigar(tb)
        if with_seq:
            ig.spill_seq(tb)
        assert np.array_equal(d_off.cpu().numpy(), tb.cig_off) and np.array_equal(d_pos.cpu().numpy(), tb.pos)
        out[int(tb.tid[0])] = tb
    return out


def _ref_end(table):
    """pos + the reference span of every record (at least 1), by the host oracle of the scan."""
    return table.pos.astype(np.int64) + np.maximum(helpers.oracle_scan(table, 50)[2][:, 0].astype(np.int64), 1)


def _windows(length, window=WINDOW):
    return [(a, min(length, a + window)) for a in range(0, length, window)]


@pytest.mark.parametrize("name", ["collect_small", "ont_small"])
def test_whole_references_table_for_table(golden, group_sizes, name):
    g, ig = golden[name], group_sizes
    for sizes in GROUP_SIZES:
        ig.FIRST_GROUP_BYTES, ig.PIPE_GROUP_BYTES = sizes
        got, want = _whole_tables(ig, g["path"], g["csi"]), _whole_tables(ig, g["path"], g["bai"])
        assert sorted(got) == sorted(want) and len(want) == (2 if name == "collect_small" else 1)
        for t in want:
            _same(got[t], want[t], (name, sizes, t))
    dec, _head = _decoder(ig, g["path"], g["csi"])
    lin, _head = _decoder(ig, g["path"], g["bai"])
    assert all(isinstance(s, csi.CsiSpan) for s in dec.spans) and all(isinstance(s, csi.LinearSpan) for s in lin.spans)
    # (the end of the last reference's records: the two writers name the same place as "behind the last byte of a block" and "the next block")
    assert [s.lo for s in dec.spans] == [s.lo for s in lin.spans] and [s.hi for s in dec.spans][:-1] == [s.hi for s in lin.spans][:-1]
    assert dec.estimate_reach() == lin.estimate_reach()


def test_with_read_bases(golden, group_sizes):
    g, ig = golden["collect_small"], group_sizes
    ig.FIRST_GROUP_BYTES, ig.PIPE_GROUP_BYTES = GROUP_SIZES[1]
    got, want = _whole_tables(ig, g["path"], g["csi"], True), _whole_tables(ig, g["path"], g["bai"], True)
    for t in want:
        _same(got[t], want[t], t)
        assert np.array_equal(np.asarray(got[t].seq_off), np.asarray(want[t].seq_off)) and got[t].seq_packed.size > 1000
        assert np.asarray(got[t].seq_packed).tobytes() == np.asarray(want[t].seq_packed).tobytes()


@pytest.mark.parametrize("name", ["collect_small", "ont_small"])
def test_small_slices_decode_their_ranges(golden, group_sizes, name):
    """Slices of one window each: the device decodes exactly the file range every unit of the .csi plan names, and that range holds
    every record that overlaps the unit's windows widened by the margin."""
    g, ig = golden[name], group_sizes
    whole = bam.read_bam(g["path"])
    ref_end = _ref_end(whole)
    for sizes in (GROUP_SIZES[0], GROUP_SIZES[2]):
        ig.FIRST_GROUP_BYTES, ig.PIPE_GROUP_BYTES = sizes
        dec, head = _decoder(ig, g["path"], g["csi"])
        margin = 32768
        units = dec.plan_units(list(range(len(head.references))), lambda t: _windows(head.lengths[t]), margin=margin, slice_bytes=1, min_span_margins=0)
        assert len(units) >= 8 and sum(not u.to_end for u in units) >= 5 and sum(u.left_edge is not None for u in units) >= 4
        got = []
        for unit, finish, _arrays in dec.units_pipelined(units):
            tb = finish()
            ig.spill_cigar(tb)
            got.append(unit)
            _same(tb, _range_table(g["path"], unit.vlo, unit.vhi), unit)
            rows = np.flatnonzero((whole.tid == unit.tid) & (whole.pos < unit.hi + margin) & (ref_end > unit.lo - margin))
            assert set(zip(whole.pos[rows].tolist(), whole.l_seq[rows].tolist())) <= set(zip(tb.pos.tolist(), tb.l_seq.tolist())), unit
            assert unit.to_end or len(tb) < int((whole.tid == unit.tid).sum())
        assert got == units


def _serve(g, idx, env, window=WINDOW):
    """Every window's Sample through ChromosomeFeed over the index ``idx`` -> ({(chrom, start): Sample}, stats)."""
    path = g["path"]
    head = bam.read_bam_header(path)
    tasks = {c: _windows(n, window) for c, n in zip(head.references, head.lengths)}
    opts = helpers.default_options(min_support=3, batch_size=64, bam_path=path, window_size=window)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        feed = ingest.ChromosomeFeed(path, bam.Fasta(sequences=g["fasta"]._seq), opts, head.references, head.references, head.lengths,
                                     device=torch.device(DEV), index=idx, threads=4, engine="gpu", tasks=tasks)
        out = {}
        try:
            for chrom, wins in tasks.items():
                for start, _end in wins:
                    _key, smp = feed.get(chrom, block=True, start=start)
                    out[(chrom, start)] = smp
            stats = dict(feed.stats)
        finally:
            feed.close()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return out, stats


@pytest.mark.parametrize("name", ["collect_small", "ont_small"])
def test_feed_every_slice_complete_on_the_first_plan(golden, name):
    """SVX_SLICE_BYTES forces slices of a window or two: from the .csi no slice is rejected (replans == 0), and every window's Sample
    holds every record that overlaps the window widened by the Sample's reach."""
    g = golden[name]
    env = {"SVX_SLICE_BYTES": "20000", "SVX_SLICE_MIN_MARGINS": "0"}
    got, stats = _serve(g, g["csi"], env)
    _want, stats_bai = _serve(g, g["bai"], env)
    assert stats["engine"] == "gpu" and stats["replans"] == 0 and stats["slices"] >= 2 and stats["slices"] >= stats_bai["slices"] - 1, (stats, stats_bai)
    whole = bam.read_bam(g["path"])
    ref_end = _ref_end(whole)
    for (chrom, start), smp in got.items():
        tid, reach, t = whole.get_tid(chrom), smp.reach(), smp.table
        rows = np.flatnonzero((whole.tid == tid) & (whole.pos < start + WINDOW + reach) & (ref_end > start - reach))
        assert set(zip(whole.pos[rows].tolist(), whole.l_seq[rows].tolist())) <= set(zip(t.pos.tolist(), t.l_seq.tolist())), (chrom, start)
    # min_shift 12: not for the device engine -- the feed says why and the host engine serves the same records
    got12, stats12 = _serve(g, g["csi12"], env)
    assert stats12["engine"] == "cpu" and stats12["records"] == len(whole)


# ---- positions from 2^29 on ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("csi_long")
    path = str(d / "long.sorted.bam")
    # (2 kb of padding a record: the file has several BGZF blocks, so that slices can end in different ones)
    recs = [dict(r, tags=r.get("tags", []) + [("XP", "Z", "p" * 2000)]) for r in csilike.long_records()]
    htslike.write_bam(path, csilike.LONG_REFS, recs, level=1, index=False)
    return path, index.build_index(path, fmt="csi")


def test_long_reference_equals_the_host_reader(long_file, group_sizes):
    path, idx = long_file
    ig = group_sizes
    assert bam.find_index(path) == idx == path + ".csi"
    whole = bam.read_bam(path)
    assert int(whole.pos.max()) > 699_990_000 and int((whole.pos >= EDGE).sum()) > 40
    for sizes in (GROUP_SIZES[0], GROUP_SIZES[2]):
        ig.FIRST_GROUP_BYTES, ig.PIPE_GROUP_BYTES = sizes
        got = _whole_tables(ig, path, idx)
        assert sorted(got) == [0, 1]
        for t in (0, 1):
            _same(got[t], whole.subset(np.flatnonzero(whole.tid == t)), (sizes, t))
    # the windows on both sides of 2^29, at 0, under the 2^27-base record and at the reference's end, each a slice of its own
    wins = {0: [(0, 100_000), (50_000_000, 50_100_000), (EDGE - 100_000, EDGE), (EDGE, EDGE + 100_000), (699_900_000, 700_000_000)], 1: _windows(600_000, 200_000)}
    dec, head = _decoder(ig, path, idx)
    margin = 32768
    units = dec.plan_units([0, 1], lambda t: wins[t], margin=margin, slice_bytes=1, min_span_margins=0)
    assert [(u.tid, w) for u in units for w in u.windows] == [(t, w) for t in (0, 1) for w in wins[t]] and len(units) >= 6
    ref_end = _ref_end(whole)
    n_seen = 0
    for unit, finish, (_d_cigar, _d_off, d_pos) in dec.units_pipelined(units):
        rows = np.flatnonzero((whole.tid == unit.tid) & (whole.pos < unit.hi + margin) & (ref_end > unit.lo - margin))
        if finish is None:
            assert rows.size == 0, unit
            continue
        tb = finish()
        ig.spill_cigar(tb)
        _same(tb, _range_table(path, unit.vlo, unit.vhi), unit)
        assert np.array_equal(d_pos.cpu().numpy(), tb.pos)
        assert set(whole.pos[rows].tolist()) <= set(tb.pos.tolist()) and rows.size, unit
        n_seen += 1
    assert n_seen == len(units)
    # the scan on such positions: reference spans and ends as the host computes them
    from svision_amd import kernels
    t0 = got[0]
    d_cigar = torch.from_numpy(np.asarray(t0.cigar).view(np.int32)).to(DEV)
    scan = kernels.cigar_scan(d_cigar, torch.from_numpy(np.asarray(t0.cig_off)).to(DEV), torch.from_numpy(t0.pos).to(DEV), 50, n_words=int(t0.cig_off[-1]))
    host = whole.subset(np.flatnonzero(whole.tid == 0))
    assert np.array_equal(np.maximum(scan.stats[:, 0].cpu().numpy().astype(np.int64), 1), _ref_end(host) - host.pos) and int(scan.stats[:, 0].max()) == 1 << 27


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_command_line_with_only_a_csi(golden, tmp_path):
    """A copy of collect_small.bam with nothing but a .csi beside it: the VCF and segments/ of the run with the .bai, at -t 1 and -t 3,
    on the device engine; with a min_shift 12 index the same files from the host engine, and the log says which engine read."""
    from oracle import alexnet_ref
    from svision_amd.network import tf_checkpoint as ck
    g = golden["collect_small"]
    prefix = str(tmp_path / "m.ckpt")
    ck.write_checkpoint(prefix, alexnet_ref.random_params(seed=7))
    fa = str(tmp_path / "collect_small.fa")
    bam.write_fasta(fa, {n: g["fasta"]._seq[n] for n in g["fasta"].references})
    inputs = {}
    for what, idx in (("bai", g["bai"]), ("csi", g["csi"]), ("csi12", g["csi12"])):
        os.mkdir(str(tmp_path / what))
        inputs[what] = str(tmp_path / what / "collect_small.bam")
        shutil.copy(g["path"], inputs[what])
        shutil.copy(idx, inputs[what] + (".bai" if what == "bai" else ".csi"))
    outs = {}
    for what, t, engine in (("bai", "1", "device"), ("csi", "1", "device"), ("csi", "3", "device"), ("csi12", "1", "host")):
        out = str(tmp_path / ("out_%s_%s" % (what, t)))
        e = {k: v for k, v in os.environ.items() if k not in ("SVX_BUILD_INDEX", "SVX_INGEST")}
        r = subprocess.run([sys.executable, os.path.join(ROOT, "SVision"), "-o", out, "-b", inputs[what], "-m", prefix, "-g", fa, "-n", "HGi", "-s", "3",
                            "--window_size", "150000", "--batch_size", "64", "--debug", "-t", t], capture_output=True, text=True, timeout=600,
                           env=dict(e, PYTHONPATH=ROOT, SVX_TIMING="1"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert ("'engine': '%s'" % ("gpu" if engine == "device" else "cpu")) in r.stdout
        log = "".join(open(os.path.join(out, f)).read() for f in os.listdir(out) if f.endswith(".log"))
        assert "records decoded by the %s engine" % engine in log and ("min_shift 12" in log) == (what == "csi12")
        outs[(what, t)] = {rel: open(os.path.join(out, rel)).read() for rel in ["HGi.svision.s3.vcf"] +
                           ["segments/" + f for f in sorted(os.listdir(os.path.join(out, "segments")))]}
    want = outs[("bai", "1")]
    assert want["HGi.svision.s3.vcf"].count("\n") > 20 and len(want) > 1
    for k, v in outs.items():
        assert v == want, k
