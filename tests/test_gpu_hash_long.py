"""svx_hash_seeds_long (svision_amd/csrc/svx_hash.hip): --hash pieces of 2,049 .. 65,536 bases on the device, x's k-mer entries in
tiles of 4,096.  The cases of tests/hashcases_long.py against the host aligner's raw hit lists (tests/hashcases.raw_hit_lists) and
the reference's final segments (tests/golden/hash_long.expected.json.gz); short and long jobs in one batch; the collection and
the command line with --max_hash_len 5000 against the host aligner's run."""
import ast
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import hashcases as hc
from tests import hashcases_long as hl
from tests import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SINGLE = {}


def single(case, k=None, window=None):
    """The kernels' lists for one job alone in its launch (once per process); k / window default to the case's own."""
    from svision_amd import kernels
    k, window = k or case.k, window or case.window
    key = (case.name, k, window)
    if key not in _SINGLE:
        res = kernels.hash_seeds([(kernels.pack_bases(case.seq), kernels.pack_bases(case.ref))], k, window, DEV, max_piece=kernels.HASH_LONG_MAX_X)[0]
        _SINGLE[key] = None if res is None else (res[0].tolist(), res[1].tolist())
    return _SINGLE[key]


def eligible():
    return [c for c in hl.all_cases() if hl.device_eligible(c)]


def test_raw_hit_lists_match_host_aligner():
    """Every case alone in a launch: both lists equal the host aligner's, order included; None (overflow) for the overflow case
    and for no other; the 65,537-base piece is refused."""
    from svision_amd import _lib, kernels
    assert len(eligible()) == len(hl.all_cases()) - 1
    for c in eligible():
        got = single(c)
        if c.name == hl.OVERFLOW:
            assert got is None
            continue
        assert got is not None, c.name
        want_a, want_b = hc.raw_hit_lists_of(c)
        assert got[0] == want_a, c.name
        assert got[1] == want_b, c.name
    c = hl.by_name()[hl.TOO_LONG]
    with pytest.raises(_lib.SvxError):
        kernels.hash_seeds([(kernels.pack_bases(c.seq), kernels.pack_bases(c.ref))], c.k, c.window, DEV, max_piece=kernels.HASH_LONG_MAX_X)
    with pytest.raises(_lib.SvxError):
        kernels.hash_seeds([(kernels.pack_bases(c.seq), kernels.pack_bases(c.ref))], c.k, c.window, DEV, max_piece=kernels.HASH_LONG_MAX_X + 1)


def test_final_segments_match_reference(monkeypatch):
    """hashplot_unmapped_batch with MAX_PIECE set (one launch per (k, window)) + the host merge == the reference; the overflow
    case and the 65,537-base piece == the reference through hashplot_unmapped's host fallback."""
    from svision_amd import kernels
    from svision_amd.segmentplot import run_hash_lineplot as rh
    monkeypatch.setattr(rh, "MAX_PIECE", kernels.HASH_LONG_MAX_X)
    monkeypatch.setattr(rh, "DEVICE", DEV)
    want = hl.load_expected()
    groups = {}
    for c in hl.all_cases():
        groups.setdefault((c.k, c.window), []).append(c)
    for (k, window), cases in groups.items():
        got = rh.hashplot_unmapped_batch([(c.ref, c.seq) for c in cases], k, window, DEV)
        for c, segs in zip(cases, got):
            if c.name in (hl.OVERFLOW, hl.TOO_LONG):
                assert segs is None, c.name
                main, segs = rh.hashplot_unmapped(c.ref, c.seq, c.k, c.window)
                assert main is None
            assert segs is not None, c.name
            assert hc.fmt(segs) == want[c.name]["segs"], c.name


def mixed_batch(k, window):
    """The long cases interleaved with 30 short jobs of tests/hashcases.py, shuffled; at k = 2 the overflowing long job stands
    between the two tile-edge jobs, which have hits of their own."""
    short = ([x for x in hc.sweep_cases() if x.k == 10] + [x for x in hc.degenerate_cases() if x.name.endswith("k10w50")]
             + [x for x in hc.tiny_cases() if x.name.startswith("b/hand/")])[:30]
    assert len(short) == 30
    trio = [hl.by_name()[n] for n in ("l/edge4096/k2w2", hl.OVERFLOW, "l/edge4098/k2w2")]
    rest = [c for c in eligible() if c not in trio]
    order = [c for pair in zip(rest, short) for c in pair] + short[len(rest):]
    random.Random(k * 100 + window).shuffle(order)
    order[len(order) // 2:len(order) // 2] = trio
    assert len(order) == len(eligible()) + 30
    return order


def same_lists(order, got, want):
    assert len(got) == len(want)
    for c, g, w in zip(order, got, want):
        if w is None:
            assert g is None, c.name
        else:
            assert g is not None, c.name
            assert (g[0].tolist(), g[1].tolist()) == w, c.name


@pytest.mark.parametrize("k,window", [(10, 50), (2, 2)])
def test_mixed_batch_equals_single_launches(k, window):
    """Short and long jobs in ONE launch pair (svx_hash_seeds and svx_hash_seeds_long over the same jobs), then the same batch
    reversed over the dirty scratch the allocator hands back, cut into three or more launches by a byte budget, and packed
    into an array of 8 rows first: every job's lists equal those of the job alone in a launch, element for element."""
    from svision_amd import kernels
    order = mixed_batch(k, window)
    want = [single(c, k, window) for c in order]
    if (k, window) == (2, 2):
        at = order.index(hl.by_name()[hl.OVERFLOW])
        assert want[at] is None and len(want[at - 1][1]) >= 5 and len(want[at + 1][1]) >= 5
    else:
        assert all(w is not None for w in want) and sum(bool(w[1]) for w in want) >= 20
        assert sum(bool(w[1]) for c, w in zip(order, want) if len(c.seq) > hc.MAX_X) >= 10
    packed = [(kernels.pack_bases(c.seq), kernels.pack_bases(c.ref)) for c in order]
    big = kernels.HASH_LONG_MAX_X
    same_lists(order, kernels.hash_seeds(packed, k, window, DEV, max_piece=big), want)
    same_lists(order[::-1], kernels.hash_seeds(packed[::-1], k, window, DEV, max_piece=big), want[::-1])
    # the 70,000-base window alone asks for 16 MB of table, 9 MB of lists and 1.3 MB of workspace; the others for about 25 MB together
    bases, desc = kernels.hash_job_arrays(packed)
    handle = kernels.hash_seeds_async(bases, desc, k, window, DEV, budget=12 << 20, max_piece=big)
    got = kernels.hash_split_rows(desc, *handle.result())
    assert handle.launches >= 3
    same_lists(order, got, want)
    handle = kernels.hash_seeds_async(bases, desc, k, window, DEV, packed_rows=8, max_piece=big)
    got = kernels.hash_split_rows(desc, *handle.result())
    assert handle.launches == 1
    same_lists(order, got, want)


def test_refusals():
    """k outside 2..13, a piece bound above 65,536 and a missing workspace are refused by the C entry point before any launch (the
    count words keep their sentinel); each kernel leaves the other's job alone."""
    import torch
    from svision_amd import _lib, kernels
    lib = _lib.load()
    c = hl.by_name()[hl.STRAND]
    x, y = kernels.pack_bases(c.seq), kernels.pack_bases(c.ref)
    desc = np.zeros(2, kernels.HASH_JOB_DTYPE)
    cap = 4 * len(y) + 64
    desc[0] = (0, len(x), len(x), len(y), 0, 32768, cap, 0)                               # the long job
    desc[1] = (0, len(x), 2000, len(y), 32768, 32768, cap, 2 * cap)                       # its first 2,000 bases: a short job
    d_bases = torch.from_numpy(np.concatenate([x, y, np.zeros(16, np.uint8)])).to(DEV)
    d_jobs = torch.from_numpy(desc.view(np.uint8).copy()).to(DEV)
    d_table = torch.zeros(2 * 32768 * 2, dtype=torch.int64, device=DEV)
    d_hits = torch.zeros(2 * 2 * cap * 4, dtype=torch.int32, device=DEV)
    d_counts = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    ws_bytes = lib.svx_hash_seeds_long_ws_bytes(len(x), len(y))
    d_ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    d_ws_off = torch.zeros(2, dtype=torch.int64, device=DEV)
    sp = kernels._stream_ptr(torch.device(DEV))

    def call_long(k, max_x, ws=True):
        rc = lib.svx_hash_seeds_long(d_bases.data_ptr(), d_jobs.data_ptr(), 2, d_table.data_ptr(), d_hits.data_ptr(), d_counts.data_ptr(),
                                     d_ws.data_ptr() if ws else None, d_ws_off.data_ptr(), k, 50, max_x, sp)
        torch.cuda.synchronize()
        return rc

    for k, max_x, ws in ((1, 65536, True), (14, 65536, True), (10, 65537, True), (10, 65536, False)):
        assert call_long(k, max_x, ws) == _lib.SVX_EINVAL, (k, max_x, ws)
        assert d_counts.tolist() == [-7] * 4
    want_a, want_b = hc.raw_hit_lists_of(c)
    assert call_long(10, 65536) == _lib.SVX_OK
    assert d_counts.tolist() == [len(want_a), len(want_b), -7, -7]                        # the short job is not this kernel's
    d_counts.fill_(-7)
    rc = lib.svx_hash_seeds(d_bases.data_ptr(), d_jobs.data_ptr(), 2, d_table.data_ptr(), d_hits.data_ptr(), d_counts.data_ptr(), 10, 50, 2048, sp)
    torch.cuda.synchronize()
    short_a, short_b = hc.raw_hit_lists(c.ref, c.seq[:2000], 10, 50)
    assert rc == _lib.SVX_OK and d_counts.tolist() == [-7, -7, len(short_a), len(short_b)]   # ... and the long job not the short kernel's


# ---- collection and command line: reads with a 3,000-base insertion, --max_hash_len 5000 -------------------------------------------
def _dump(sigs):
    return [[s.type, s.tstart, s.tend, s.qname, s.bkps, s.mechanism,
             [[a.q_start, a.q_end, a.ref_start, a.ref_end, bool(a.is_reverse)] for a in s.sorted_aligns]] for s in sigs]


def test_collection_long_pieces_device_equals_host(tmp_path, monkeypatch):
    """detect_window --hash --max_hash_len 5000 on the sample of hashcases_long.sample_table (written and read back with the
    repository's own BAM writer): the device run with MAX_PIECE set and the host aligner (rh.DEVICE = None) give the same
    signatures and TSV, and the six 3,000-base and the six 2,500-base insertions reach kernels.hash_seeds.  The yardstick is the host path.
    The 2,500 unaligned bases between the split reads' two alignments reach the re-aligner as EMPTY pieces in both runs: the
    collection keeps upstream's slicing of the segment's own bases with whole-read coordinates (analyze_reads._hash_between)."""
    from svision_amd import kernels
    from svision_amd.collection.output_clusters import collect_pair_lines
    from svision_amd.collection.run_collection import detect_window
    from svision_amd.io import bam
    from svision_amd.sample import Sample
    from svision_amd.segmentplot import run_hash_lineplot as rh
    table, seqs = hl.sample_table()
    path = str(tmp_path / "long.bam")
    bam.write_bam(path, table, index=True)
    assert len(table) == 24
    seen, orig = [], kernels.hash_seeds

    def spy(jobs, *a, **kw):
        seen.append(([len(x) for x, _y in jobs], kw.get("max_piece")))
        return orig(jobs, *a, **kw)

    monkeypatch.setattr(kernels, "hash_seeds", spy)
    results = []
    for on_device in (True, False):
        sample = Sample.from_table(bam.read_bam(path, with_seq=True), bam.Fasta(sequences=seqs), 50, device=DEV)
        assert rh.DEVICE is not None
        monkeypatch.setattr(rh, "MAX_PIECE", kernels.HASH_LONG_MAX_X if on_device else None)
        if not on_device:
            monkeypatch.setattr(rh, "DEVICE", None)
        before = len(seen)
        opts = helpers.default_options(min_support=3, hash=True, max_hash_len=5000)
        sigs, clusters = detect_window(opts, sample, hl.SAMPLE_CHROM, 0, hl.SAMPLE_LEN)
        assert (len(seen) > before) == on_device
        results.append((_dump(sigs), "".join(p.text() for p in collect_pair_lines(clusters, opts))))
    assert len(seen) == 1 and seen[0][1] == kernels.HASH_LONG_MAX_X
    assert sorted(seen[0][0]) == [0] * 6 + [hl.SAMPLE_INS2] * 6 + [hl.SAMPLE_INS] * 6                    # jobs over 2,048 bases reached the device
    assert results[0][0] == results[1][0]
    assert results[0][1] == results[1][1]
    assert sum(1 for d in results[0][0] if len(d[6]) > 2) >= 12 and results[0][1].count("\n") > 10      # the insertions were placed


def _outputs(out):
    seg = os.path.join(out, "segments")
    files = {f: open(os.path.join(seg, f), "rb").read() for f in sorted(os.listdir(seg))}
    return open(os.path.join(out, "HGl.svision.s3.vcf"), "rb").read(), files


@pytest.mark.parametrize("threads", [1, 3])
def test_command_line_long_pieces(tmp_path, threads):
    """./SVision --hash --max_hash_len 5000 on that sample: VCF and segments/ are byte for byte those of the same run under
    SVX_HASH_LONG=0 (the long pieces through the host aligner); with helpers, the owner's profile counts the long jobs among the
    helpers' requests and no request failed."""
    from oracle import alexnet_ref
    from svision_amd.io import bam
    from svision_amd.network import tf_checkpoint as ck
    prefix = str(tmp_path / "m.ckpt")
    ck.write_checkpoint(prefix, alexnet_ref.random_params(seed=7))
    table, seqs = hl.sample_table()
    path, fa = str(tmp_path / "long.bam"), str(tmp_path / "long.fa")
    bam.write_bam(path, table, index=True)
    bam.write_fasta(fa, seqs)
    outs, profs = {}, {}
    for long_on in ("1", "0"):
        out = str(tmp_path / ("out" + long_on))
        env = {k: v for k, v in os.environ.items() if k not in ("SVX_HASH_LONG", "SVX_HASH_BATCH", "SVX_INGEST")}
        r = subprocess.run([sys.executable, os.path.join(ROOT, "SVision"), "-o", out, "-b", path, "-m", prefix, "-g", fa, "-n", "HGl", "-s", "3",
                            "--hash", "--max_hash_len", "5000", "--batch_size", "64", "--debug", "-t", str(threads)],
                           capture_output=True, text=True, timeout=600, env=dict(env, PYTHONPATH=ROOT, SVX_TIMING="1", SVX_HASH_LONG=long_on))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        outs[long_on] = _outputs(out)
        m = re.search(r"owner (\{.*\})", r.stdout)
        profs[long_on] = ast.literal_eval(m.group(1)) if m else None
    assert outs["1"][0] == outs["0"][0] and outs["1"][0].count(b"\n") > 20
    assert outs["1"][1] == outs["0"][1] and sum(len(v) for v in outs["1"][1].values()) > 1000
    if threads > 1:
        on, off = profs["1"], profs["0"]
        assert on.get("hash.failed", 0) == 0 and off.get("hash.failed", 0) == 0
        assert on["hash.requests"] >= 1 and on["hash.launches"] >= 1
        assert on["hash.jobs"] - off["hash.jobs"] == 12                    # the long insertions: in the requests only with the long kernel
