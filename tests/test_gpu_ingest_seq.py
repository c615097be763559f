"""The device ingest engine WITH the read bases (-m gpu): svx_bam_walk_count_seq / svx_bam_walk_extract_seq behind
ingest_gpu.DeviceDecoder(with_seq=True), the lazy bases (LazySeq + the spill thread) behind ingest.ChromosomeFeed, and the two
command-line modes that want them -- ``--hash`` and ``--graph --qname`` -- on the device engine.  The yardstick is the host
decoder (svx_bam.cpp parse_records): l_seq, seq_off and the bytes of seq_packed are equal element for element."""
import gzip
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from svision_amd import ingest, synth
from svision_amd.io import bam
from tests import helpers, htslike

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = 100_000
GROUP_SIZES = ((1 << 10, 1 << 10), (1 << 20, 3 << 20), (1 << 40, 1 << 40))        # test_pipelined_device_decoder_equals_the_host_decoder's


@pytest.fixture(autouse=True)
def _restore_group_sizes():
    import svision_amd.ingest_gpu as ig
    saved = ig.FIRST_GROUP_BYTES, ig.PIPE_GROUP_BYTES, ig.LARGE_GROUP_BYTES
    yield
    ig.FIRST_GROUP_BYTES, ig.PIPE_GROUP_BYTES, ig.LARGE_GROUP_BYTES = saved


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _simulated(tmp_path):
    """Several contigs with synthesised bases (primaries carry SEQ, the others SEQ = *), written by the plain writer + its .bai."""
    cfg = synth.SimConfig(contigs=[("s1", 300_000), ("s2", 120_000), ("s3", 200_000)], coverage=8, read_len_mean=5000, read_len_sd=900,
                          sv_spacing=9000, sv_min_gap=5000, sv_max=1500, seed=31)
    table, _genome, _ = synth.simulate(cfg, with_seq=True)
    path = str(tmp_path / "sim.bam")
    bam.write_bam(path, table, index=True)
    return path


def _segments(tmp_path, name, contigs, read_len, sd, coverage, seed):
    """encode_reference_segment(seq="random"): the bench's writer -- 64 KB blocks, records straddle them."""
    cfg = synth.SimConfig(contigs=contigs, coverage=coverage, read_len_mean=read_len, read_len_sd=sd, sv_spacing=20_000, sv_min_gap=9_000,
                          sv_max=3000, seed=seed)
    table, _g, _ = synth.simulate(cfg, with_genome=False)
    tids = sorted(set(table.tid.tolist()))
    segs = [bam.encode_reference_segment(table.subset(np.flatnonzero(table.tid == t)), seq="random", seed=t) for t in tids]
    path = str(tmp_path / (name + ".bam"))
    bam.write_bam_segments(path, table.references, table.lengths, segs)
    return path


def _htslike(tmp_path, policy):
    """Records written by the independent writer: SEQ = *, reads of 1 and 2 bases, odd and even lengths, tags, and a record
    of 66,000 CIGAR operations (CG:B,I tag + placeholder) WITH its bases."""
    rng = np.random.default_rng(5 if policy == "htslib" else 6)

    def seq(n):
        return "".join("ACGTN"[i] for i in rng.integers(0, 5, n))
    refs = [("h1", 400_000), ("h2", 250_000)]
    recs = []
    for tid, (_name, length) in enumerate(refs):
        for i in range(260):
            n = int(rng.integers(40, 3000))
            pos = int(rng.integers(0, length - 70_000))
            kind = i % 13
            rec = {"tid": tid, "pos": pos, "qname": "r%d_%d" % (tid, i), "flag": 16 if i % 3 == 0 else 0, "mapq": 60}
            if kind == 0:
                rec.update(cigar=[(n, "M")], seq="*")                                   # SEQ absent
            elif kind == 1:
                rec.update(cigar=[(1, "M")], seq=seq(1))
            elif kind == 2:
                rec.update(cigar=[(2, "M")], seq=seq(2))
            elif kind == 3:
                rec.update(cigar=[(5, "S"), (n, "M"), (7, "I"), (20, "M")], seq=seq(n + 32), qual=bytes(rng.integers(0, 40, n + 32).tolist()),
                           tags=[("NM", "i", 3), ("MD", "Z", "10A5"), ("ML", "BC", [1, 2, 3])])
            else:
                rec.update(cigar=[(n, "M")], seq=seq(n), tags=[("RG", "Z", "rg1")] if i % 2 else [])
            recs.append(rec)
    n_ops = 66_000
    recs.append({"tid": 1, "pos": 1000, "qname": "long_cigar_read", "flag": 0, "mapq": 60, "cigar": [(1, "=X"[i & 1]) for i in range(n_ops)],
                 "seq": seq(n_ops)})
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    path = str(tmp_path / ("hts_%s.bam" % policy))
    htslike.write_bam(path, refs, recs, level=6 if policy == "htslib" else 1, policy=policy)
    return path


def _device_tables(path, group_sizes):
    """{tid: table} of DeviceDecoder(with_seq=True).parts_pipelined, words and bases spilled to the host."""
    import svision_amd.ingest_gpu as ig
    ig.FIRST_GROUP_BYTES, ig.PIPE_GROUP_BYTES = group_sizes
    head = bam.read_bam_header(path)
    dec = ig.DeviceDecoder(path, bam.find_index(path), head.references, head.lengths, head.header_text, "cuda:0", threads=3, with_seq=True)
    tids = list(range(len(head.references)))
    assert dec.usable(tids)
    out = {}
    for finish, (_d_cigar, d_off, _d_pos) in dec.parts_pipelined(tids):
        tb = finish()
        assert type(tb.seq_packed).__name__ == "LazySeq"
        if tb.seq_packed.size:
            with pytest.raises(RuntimeError):
                tb.seq_packed[0]                               # the bases are on the device only ...
        ig.spill_cigar(tb)
        ig.spill_seq(tb)                                       # ... until the feed's spill thread has copied them out
        assert np.array_equal(d_off.cpu().numpy(), tb.cig_off)
        out[int(tb.tid[0])] = tb
    return out, head


def _facts(host):
    """What a host table holds of the shapes the copy kernel must get right."""
    l_seq = host.l_seq.astype(np.int64)
    off = np.asarray(host.seq_off, np.int64)
    both = (l_seq[1:] > 0) & (l_seq[:-1] > 0)
    n_cig = np.diff(host.cig_off)
    return {"star": int((l_seq == 0).sum()), "one": int((l_seq == 1).sum()), "two": int((l_seq == 2).sum()),
            "odd": int(((l_seq & 1) == 1).sum()), "even": int(((l_seq > 0) & ((l_seq & 1) == 0)).sum()),
            "cg_with_bases": int(((n_cig > 65535) & (l_seq > 0)).sum()),
            "unaligned_boundaries": int((both & (off[1:] % 16 != 0)).sum())}


def test_device_decoder_with_bases_equals_the_host_decoder(tmp_path):
    paths = [_simulated(tmp_path),
             _segments(tmp_path, "seg", [("c%d" % i, 260_000 + 70_000 * (i % 3)) for i in range(5)], 9000, 1500, 8, 21),
             # ONT-shaped: a record of ~150 kb is 75 KB of SEQ + 150 KB of QUAL -- four BGZF blocks
             _segments(tmp_path, "ont", [("o1", 2_000_000), ("o2", 1_200_000)], 150_000, 30_000, 5, 77),
             _htslike(tmp_path, "htslib"), _htslike(tmp_path, "stream")]
    total = {}
    for path in paths:
        for sizes in GROUP_SIZES:
            got, head = _device_tables(path, sizes)
            want_tids = []
            for t in range(len(head.references)):
                host = bam.read_bam(path, with_seq=True, tids=[t], index=bam.find_index(path))
                if len(host) == 0:
                    assert t not in got
                    continue
                want_tids.append(t)
                dev = got[t]
                assert np.array_equal(dev.l_seq, host.l_seq), (path, t)
                assert np.asarray(dev.seq_off).dtype == np.int64 and np.array_equal(np.asarray(dev.seq_off), np.asarray(host.seq_off)), (path, t)
                assert dev.seq_packed.size == len(host.seq_packed)
                assert np.asarray(dev.seq_packed).tobytes() == bytes(host.seq_packed), (path, t)
                for f in ("tid", "pos", "flag", "mapq", "cig_off"):
                    assert np.array_equal(getattr(dev, f), getattr(host, f)), f
                assert np.array_equal(np.asarray(dev.cigar), host.cigar)
                rows = np.unique(np.concatenate([np.arange(min(len(host), 40)), np.flatnonzero(host.l_seq <= 2)]))
                for i in rows.tolist():
                    assert dev.query_sequence(i) == host.query_sequence(i)
                sub = dev.subset(rows)                          # the lazy form goes through subset as it is
                assert [sub.query_sequence(j) for j in range(len(sub))] == [host.query_sequence(i) for i in rows.tolist()]
                if sizes == GROUP_SIZES[0]:
                    for k, v in _facts(host).items():
                        total[k] = total.get(k, 0) + v
            assert sorted(got) == want_tids
    # together the inputs hold every shape the issue names
    assert total["star"] >= 1 and total["one"] >= 1 and total["two"] >= 1 and total["odd"] >= 1 and total["even"] >= 1, total
    assert total["cg_with_bases"] >= 1, total
    assert total["unaligned_boundaries"] >= 1000, total        # dense offsets: nearly every pair of neighbours shares a 16-byte chunk


# ---- the feed -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sliced_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ingest_seq")
    cfg = synth.SimConfig(contigs=[("chrA", 1_500_000), ("chrB", 250_000), ("chrC", 700_000)], coverage=14, read_len_mean=8000, read_len_sd=1500,
                          err_rate=0.004, sv_spacing=9_000, sv_min_gap=6_000, sv_max=3000, inline_max=1200, seed=78)
    table, genome, _svs = synth.simulate(cfg)
    path = str(d / "s.bam")
    segs = [bam.encode_reference_segment(table.subset(np.flatnonzero(table.tid == t)), seq="random", seed=t) for t in range(3)]
    bam.write_bam_segments(path, table.references, table.lengths, segs)
    return path, genome


def _windows(length):
    return [(a, min(length, a + WINDOW)) for a in range(0, length, WINDOW)]


def _sequences(table):
    """{(QNAME, pos, flag): query_sequence} of every record."""
    return {(table.names[int(table.name_id[i])], int(table.pos[i]), int(table.flag[i])): table.query_sequence(i) for i in range(len(table))}


def test_feed_serves_slices_with_their_bases(sliced_files):
    path, genome = sliced_files
    head = bam.read_bam_header(path)
    fasta = bam.Fasta(sequences=genome)
    tasks = {c: _windows(n) for c, n in zip(head.references, head.lengths)}
    whole = bam.read_bam(path, with_seq=True)
    want = {}
    for t, chrom in enumerate(head.references):
        want[chrom] = _sequences(whole.subset(np.flatnonzero(whole.tid == t)))
        assert sum(v is not None for v in want[chrom].values()) > 100
    opts = helpers.default_options(min_support=3, batch_size=64, bam_path=path, window_size=WINDOW, hash=True)
    env = {"SVX_SLICE_BYTES": "200000", "SVX_SLICE_MIN_MARGINS": "0"}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        feed = ingest.ChromosomeFeed(path, fasta, opts, head.references, head.references, head.lengths, device=torch.device("cuda:0"),
                                     index=bam.find_index(path), threads=4, engine="gpu", tasks=tasks)
        try:
            for chrom, wins in tasks.items():
                for start, _end in wins:
                    feed.get(chrom, block=True, start=start)
            stats = dict(feed.stats)
            assert stats["engine"] == "gpu"                    # (the parent forced "cpu" on every run that wants bases)
            assert stats["slices"] > 8 and stats["replans"] == 0
            n_checked = 0
            for chrom in head.references:
                for _lo, _hi, _key, smp, meta in feed.samples[chrom]:
                    t = smp.table
                    assert type(t.seq_packed).__name__ == "LazySeq" and meta["lazy_seq"] == t.seq_packed.size
                    got = _sequences(t)                        # the owner's view: waits for the spill's event
                    assert len(got) == len(t) > 0
                    for key, s in got.items():
                        assert s == want[chrom][key], (chrom, key)
                    # the helpers' view: what load_shared_sample maps from the announced meta (without the owner-side event)
                    sent = {a: b for a, b in meta.items() if a != "spilled"}
                    ht = ingest.load_shared_sample(sent, fasta).table
                    assert type(ht.seq_packed).__name__ == "LazySeq" and ht.seq_packed.path.endswith("seq_packed.bin")
                    assert _sequences(ht) == got
                    assert np.asarray(ht.seq_packed).tobytes() == np.asarray(t.seq_packed).tobytes()
                    n_checked += len(got)
            assert n_checked > 3000
        finally:
            feed.close()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def test_feed_falls_back_to_the_host_engine_with_bases(tmp_path):
    """A damaged linear-index entry of the second reference under --hash (the construction of
    test_feed_falls_back_to_the_host_engine_where_the_device_engine_refuses): the host engine serves that reference WITH its
    bases, the device engine the one behind it, and every table equals the host-only run's."""
    cfg = synth.SimConfig(contigs=[("c1", 300_000), ("c2", 200_000), ("c3", 250_000)], coverage=6, read_len_mean=4000, read_len_sd=600,
                          sv_spacing=9000, sv_min_gap=5000, sv_max=1000, seed=21)
    table, genome, _ = synth.simulate(cfg, with_seq=True)
    path = str(tmp_path / "fb.bam")
    bam.write_bam(path, table, index=True)
    raw = bytearray(open(path + ".bai", "rb").read())
    at = 8                                                        # magic, n_ref
    for ref in range(2):                                          # walk to reference 1's linear index
        n_bin, = struct.unpack_from("<i", raw, at); at += 4
        for _ in range(n_bin):
            _bin, n_chunk = struct.unpack_from("<Ii", raw, at); at += 8 + 16 * n_chunk
        n_intv, = struct.unpack_from("<i", raw, at); at += 4
        if ref == 0:
            at += 8 * n_intv
    vals = list(struct.unpack_from("<%dQ" % n_intv, raw, at))
    k = max(i for i in range(n_intv) if vals[i] and vals[i] != vals[-1])    # an entry in the middle of the reference's records
    struct.pack_into("<Q", raw, at + 8 * k, vals[k] + 5)          # five bytes into the record it pointed at
    bad = str(tmp_path / "bad.bam")
    shutil.copy(path, bad)
    with open(bad + ".bai", "wb") as f:
        f.write(raw)

    def serve(p, engine):
        head = bam.read_bam_header(p)
        opts = helpers.default_options(min_support=3, batch_size=64, bam_path=p, hash=True)
        feed = ingest.ChromosomeFeed(p, bam.Fasta(sequences=genome), opts, head.references, head.references, head.lengths,
                                     device=torch.device("cuda:0"), index=bam.find_index(p), threads=4, engine=engine)
        out = {}
        try:
            for chrom in head.references:
                _key, smp = feed.get(chrom, block=True)
                t = smp.table
                out[chrom] = (t.pos.copy(), t.flag.copy(), t.l_seq.copy(), np.asarray(t.seq_off).copy(), np.asarray(t.seq_packed).tobytes(),
                              [t.query_sequence(i) for i in range(len(t))], np.asarray(t.cigar).copy(), type(t.seq_packed).__name__)
                feed.release(chrom)
        finally:
            feed.close()
        return out, dict(feed.stats)
    want, _ = serve(path, "cpu")
    got, stats = serve(bad, "gpu")
    assert stats["engine"] == "gpu"
    assert got["c2"][-1] != "LazySeq" and got["c3"][-1] == "LazySeq"      # who decoded what
    for chrom in want:
        assert sum(s is not None for s in want[chrom][5]) > 20
        for a, b in zip(got[chrom][:-1], want[chrom][:-1]):
            assert (a == b) if isinstance(a, (list, bytes)) else np.array_equal(a, b), chrom


# ---- the command line -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from oracle import alexnet_ref
    from svision_amd.network import tf_checkpoint as ck
    prefix = str(tmp_path_factory.mktemp("ckpt") / "svision-cnn-model.ckpt")
    ck.write_checkpoint(prefix, alexnet_ref.random_params(seed=7))
    return prefix


def _cli(args, env):
    return subprocess.run([sys.executable, os.path.join(ROOT, "SVision")] + list(args), capture_output=True, text=True, timeout=900,
                          env=dict(os.environ, PYTHONPATH=ROOT, SVX_TIMING="1", **env))


def _indexed_golden(tmp_path, name):
    """The golden BAM with its bases, written again WITH an index, and its genome as a FASTA file."""
    fasta = helpers.load_golden_fasta(name + ".fa.gz")
    fa = str(tmp_path / (name + ".fa"))
    bam.write_fasta(fa, {n: fasta._seq[n] for n in fasta.references})
    path = str(tmp_path / (name + ".bam"))
    bam.write_bam(path, bam.read_bam(os.path.join(helpers.GOLDEN, name + ".bam"), with_seq=True), index=True)
    return path, fa


def _tree(out, rels):
    got = {}
    for rel in rels:
        p = os.path.join(out, rel)
        if os.path.isdir(p):
            for f in sorted(os.listdir(p)):
                got[rel + "/" + f] = open(os.path.join(p, f)).read()
        else:
            got[rel] = open(p).read()
    return got


def test_command_line_hash_on_the_device_engine(checkpoint, tmp_path):
    path, fa = _indexed_golden(tmp_path, "hash_collect")
    outs = {}
    for engine, t in (("cpu", "1"), ("gpu", "1"), ("gpu", "3")):
        out = str(tmp_path / ("hash_%s_%s" % (engine, t)))
        r = _cli(["-o", out, "-b", path, "-m", checkpoint, "-g", fa, "-n", "HGhash", "-s", "3", "--hash", "--batch_size", "64", "--debug", "-t", t],
                 {"SVX_INGEST": engine})
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert ("'engine': '%s'" % engine) in r.stdout, r.stdout[-3000:]
        assert "on the host" not in r.stderr
        rels = ["segments"] + (["HGhash.svision.s3.vcf"] if os.path.exists(os.path.join(out, "HGhash.svision.s3.vcf")) else [])
        outs[(engine, t)] = _tree(out, rels)
    assert outs[("cpu", "1")] == outs[("gpu", "1")] == outs[("gpu", "3")]
    with open(os.path.join(helpers.GOLDEN, "hash_collect.expected.json")) as f:
        want = [w for w in json.load(f)["windows"] if w["hash"]][0]
    assert outs[("gpu", "1")]["segments/chrH.segments.all.bed"] == want["tsv"]      # (its 53 re-aligned signatures: the bases were read)


def test_command_line_graph_on_the_device_engine(checkpoint, tmp_path):
    path, fa = _indexed_golden(tmp_path, "graph_small")
    with gzip.open(os.path.join(helpers.GOLDEN, "graph_small.expected.json.gz"), "rt") as f:
        want = json.load(f)
    args = ["-b", path, "-m", checkpoint, "-g", fa, "-n", "HGg", "-s", "3", "--window_size", str(want["window"]), "--batch_size", "64", "--qname",
            "--debug"]
    r = _cli(["-o", str(tmp_path / "plain")] + args, {"SVX_INGEST": "cpu"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    body = [l for l in open(str(tmp_path / "plain" / "HGg.svision.s3.vcf")).read().splitlines() if not l.startswith("#")]
    outs = {}
    for engine, t in (("cpu", "1"), ("gpu", "1"), ("gpu", "3")):
        out = str(tmp_path / ("graph_%s_%s" % (engine, t)))
        r = _cli(["-o", out, "--graph", "-t", t] + args, {"SVX_INGEST": engine})
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert ("'engine': '%s'" % engine) in r.stdout, r.stdout[-3000:]
        assert "on the host" not in r.stderr
        outs[(engine, t)] = _tree(out, ["HGg.svision.s3.graph.vcf", "HGg.graph_exactly_match.txt", "HGg.graph_symmetry_match.txt", "graphs", "segments"])
    assert outs[("cpu", "1")] == outs[("gpu", "1")] == outs[("gpu", "3")]
    # against the golden fixture, as tests/test_gpu_pipeline.py compares it: the collection's TSV is the reference's, the graph
    # VCF is the plain VCF's records, each with its GraphID / GFA_* fields, and one .gfa per complex record
    got = outs[("gpu", "1")]
    assert got["segments/chrG.segments.all.bed"] == "".join(w["tsv"] for w in want["windows"])
    lines = [l for l in got["HGg.svision.s3.graph.vcf"].splitlines() if not l.startswith("#")]
    assert len(lines) == len(body) >= 1
    for a, b in zip(lines, body):
        ca, cb = a.split("\t"), b.split("\t")
        assert ca[:7] == cb[:7] and ca[8:] == cb[8:] and ca[7].startswith(cb[7] + ";GraphID=")
        assert ("GraphID=-1;GFA_ID=.;GFA_S=.;GFA_L=." in ca[7]) == ("CSV" not in b)
    gfa = [k for k in got if k.startswith("graphs/")]
    assert all(k.endswith(".gfa") for k in gfa) and len(gfa) == sum("CSV" in b for b in body)
