"""--hash, a window's re-alignments as one batch (collect_signatures.analyze_alignments in two phases,
run_hash_lineplot.hashplot_unmapped_many) and the helpers' "hash" / "hashres" messages (pipeline._worker_main), without a
device: against the reference's own run (tests/golden/hash_collect.expected.json) and against the sequential collection
(SVX_HASH_BATCH=0)."""
import json
import os

import numpy as np
import pytest

from tests import hashcases as hc
from tests import helpers

SYMBOLS = "ACGTNacgtnRYKMS"                      # kernels.pack_bases


def _dump(sigs):
    return [[s.type, s.tstart, s.tend, s.qname, s.bkps, s.mechanism,
             [[a.q_start, a.q_end, a.ref_start, a.ref_end, bool(a.is_reverse)] for a in s.sorted_aligns]] for s in sigs]


def _collect(hash_on, sample=None):
    from svision_amd.collection.output_clusters import collect_pair_lines
    from svision_amd.collection.run_collection import detect_window
    from svision_amd.io import bam
    from svision_amd.sample import Sample
    if sample is None:
        table = bam.read_bam(os.path.join(helpers.GOLDEN, "hash_collect.bam"), with_seq=True)
        sample = Sample.with_scan(table, helpers.load_golden_fasta("hash_collect.fa.gz"), 50, helpers.oracle_scan(table, 50))
    opts = helpers.default_options(min_support=3, hash=hash_on)
    sigs, clusters = detect_window(opts, sample, "chrH", 0, 160_000)
    return _dump(sigs), "".join(p.text() for p in collect_pair_lines(clusters, opts))


@pytest.fixture()
def expected():
    with open(os.path.join(helpers.GOLDEN, "hash_collect.expected.json")) as f:
        return {w["hash"]: w for w in json.load(f)["windows"]}


@pytest.fixture()
def stand_in(monkeypatch):
    """hashplot_unmapped_batch replaced: -> the list of its calls; ``calls.every`` = 2 answers None for every second pair."""
    from svision_amd.segmentplot import run_hash_lineplot as rh
    monkeypatch.delenv("SVX_HASH_BATCH", raising=False)

    class Calls(list):
        every = 1

    calls = Calls()

    def batch(pairs, k, min_accept, device):
        calls.append((list(pairs), k, min_accept, device))
        return [None if calls.every == 2 and n % 2 else rh._hashplot_host(ref, seq, k, min_accept) for n, (ref, seq) in enumerate(pairs)]

    monkeypatch.setattr(rh, "hashplot_unmapped_batch", batch)
    return calls


def test_two_phase_collection_equals_reference(oracle_lib, expected, stand_in):
    """One batch call per window, carrying all 51 pieces; signatures and TSV are the reference's."""
    sigs, tsv = _collect(True)
    assert sigs == expected[True]["signatures"]
    assert tsv == expected[True]["tsv"]
    assert len(stand_in) == 1
    pairs, k, min_accept, device = stand_in[0]
    assert len(pairs) == 51 and (k, min_accept, device) == (10, 50, None)
    assert max(len(seq) for _ref, seq in pairs) == 771 and all(isinstance(r, str) and isinstance(q, str) for r, q in pairs)


def test_pairs_the_batch_refuses_run_on_the_host(oracle_lib, expected, stand_in):
    stand_in.every = 2
    sigs, tsv = _collect(True)
    assert sigs == expected[True]["signatures"]
    assert tsv == expected[True]["tsv"]
    assert len(stand_in) == 1 and len(stand_in[0][0]) == 51


def test_without_hash_no_batch(oracle_lib, expected, stand_in):
    sigs, tsv = _collect(False)
    assert sigs == expected[False]["signatures"] and tsv == expected[False]["tsv"]
    assert stand_in == []


def test_switch_off_is_the_sequential_collection(oracle_lib, expected, stand_in, monkeypatch):
    monkeypatch.setenv("SVX_HASH_BATCH", "0")
    sigs, tsv = _collect(True)
    assert sigs == expected[True]["signatures"] and tsv == expected[True]["tsv"]
    assert stand_in == []


def test_a_failing_window_contributes_nothing(oracle_lib, stand_in, monkeypatch):
    """An exception in the second phase leaves the window empty, as one in the per-read loop does."""
    from svision_amd import pipeline
    from svision_amd.io import bam
    from svision_amd.sample import Sample
    from svision_amd.segmentplot import run_hash_lineplot as rh

    def broken(pairs, k, min_accept, device):
        raise ValueError("start out of range (-1)")

    monkeypatch.setattr(rh, "hashplot_unmapped_batch", broken)
    table = bam.read_bam(os.path.join(helpers.GOLDEN, "hash_collect.bam"), with_seq=True)
    sample = Sample.with_scan(table, helpers.load_golden_fasta("hash_collect.fa.gz"), 50, helpers.oracle_scan(table, 50))
    assert pipeline._collect_lines(sample, helpers.default_options(min_support=3, hash=True), "chrH", 0, 160_000) == []


# ---- order under ties ---------------------------------------------------------------------------------------------------------
def _tie_sample():
    """One read, one alignment 100M 200I 1M 210I 100M at chrT:1000.  analyze_inside_align cuts it into the pieces
    (0,100) (301,302) (513,613) on the read, and re-aligns the insertions at read positions 100 and 301."""
    from svision_amd.io import bam
    from svision_amd.sample import Sample
    rng = np.random.default_rng(11)
    ref = "".join(rng.choice(list("ACGT"), 5000))
    read = "".join(rng.choice(list("ACGT"), 611))
    cigar = np.array([100 << 4, 200 << 4 | 1, 1 << 4, 210 << 4 | 1, 100 << 4], np.uint32)
    packed = np.frombuffer(bam.pack_sequence(read), np.uint8)
    table = bam.AlignmentTable(["chrT"], [5000], [0], [1000], [0], [60], [611], [0], ["tie"], cigar, [0, 5], "@HD\tVN:1.6\tSO:coordinate\n",
                               seq_packed=packed, seq_off=np.array([0], np.int64))
    return Sample.with_scan(table, bam.Fasta(sequences={"chrT": ref}), 50, helpers.oracle_scan(table, 50))


def _tie_hits(ref, seq):
    """Stand-in aligner: whichever insertion is asked for, two hits that land on read positions (301, 302) -- the middle
    piece's -- and one elsewhere; told apart by their reference positions."""
    from svision_amd.segmentplot.classes import Segment
    first = len(seq) == 200                      # the insertion at read position 100; the other one lies at 301
    x = 201 if first else 0
    y = 10 if first else 20
    return [Segment(x, y, 2, True, 0), Segment(x + 30, y + 1, 60, True, 0), Segment(x, y + 2, 2, True, 0)]


def test_helper_segments_that_tie_keep_their_place(oracle_lib, monkeypatch):
    """by_read_pos ties between a main piece, helper segments of the first and of the second job: the stable sort keeps the
    append order, so the two-phase list must be built exactly like the sequential one (pieces, then job 1's, then job 2's)."""
    from svision_amd.collection import analyze_reads
    from svision_amd.collection.collect_signatures import analyze_alignments
    from svision_amd.segmentplot import run_hash_lineplot as rh
    opts = helpers.default_options(min_support=1, hash=True)
    seen = []
    monkeypatch.setattr(analyze_reads, "hashplot_unmapped", lambda ref, seq, k, w: (None, _tie_hits(ref, seq)))
    monkeypatch.setattr(rh, "hashplot_unmapped_batch",
                        lambda pairs, k, w, dev: (seen.append(len(pairs)), [_tie_hits(r, s) for r, s in pairs])[1])
    got = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SVX_HASH_BATCH", mode)
        got[mode] = _dump(analyze_alignments(np.arange(1), _tie_sample(), opts))
    assert seen == [2]                                                   # the sequential run never asked the batch
    assert got["0"] == got["1"] and len(got["0"]) >= 2
    # the tie is really there (trim_segs has moved the coordinates, not the order): the four two-base hits share one read
    # interval in the second signature and stand in append order -- job 1's two (reference 1010, 1012), then job 2's
    tied = [a for a in got["1"][1][6] if a[1] - a[0] == 1]
    assert len(tied) == 4 and len({(a[0], a[1]) for a in tied}) == 1
    assert [a[2] for a in tied] == [1010, 1012, 1020, 1022]


# ---- the helper's side of the pipe ------------------------------------------------------------------------------------------
def _answer(msg):
    """The owner's reply to a helper's "hash" message, from the host aligner's raw lists."""
    _t, wid, k, window, bases, desc = msg
    assert bases.dtype == np.uint8 and desc.dtype == np.int64 and desc.shape[1] == 4
    counts, rows = [], []
    for x_off, x_len, y_off, y_len in desc.tolist():
        seq = "".join(SYMBOLS[c] for c in bases[x_off:x_off + x_len])
        ref = "".join(SYMBOLS[c] for c in bases[y_off:y_off + y_len])
        for hits in hc.raw_hit_lists(ref, seq, k, window):
            counts.append(len(hits))
            rows += hits
    row_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return ("hashres", wid, np.asarray(counts, np.uint32), row_off, np.asarray(rows, np.int32).reshape(-1, 4))


def _play_owner(monkeypatch, batch, refuse=False):
    """One helper, one window of hash_collect.bam; -> (messages of the helper in order, "hash" messages seen)."""
    from svision_amd import pipeline
    from svision_amd.io import bam
    from svision_amd.sample import Sample
    monkeypatch.setenv("SVX_HASH_BATCH", batch)
    table = bam.read_bam(os.path.join(helpers.GOLDEN, "hash_collect.bam"), with_seq=True)
    sample = Sample.with_scan(table, helpers.load_golden_fasta("hash_collect.fa.gz"), 50, helpers.oracle_scan(table, 50))
    pool = pipeline.HelperPool(1, helpers.default_options(min_support=3, hash=True), sample=sample)
    conn = pool.conns[0]
    out, asked = [], []
    try:
        conn.send(("win", 7, None, "chrH", 0, 160_000, None))
        while True:
            assert conn.poll(120), "the helper does not answer"
            msg = conn.recv()
            if msg[0] == "hash":
                asked.append(msg)
                conn.send(("opt", "want_tsv", True))                     # control messages overtake the reply ...
                conn.send(("drop", "no-such-chromosome"))
                conn.send(("hashres", msg[1], None, None, None) if refuse else _answer(msg))
                continue
            out.append(msg)
            if msg[0] == "rec":
                break
        n = msg[2]
        conn.send(("pred", 7, np.zeros(n, np.int64), np.full((n, 5), 0.2, np.float32), True))
        assert conn.poll(120)
        done = conn.recv()
    finally:
        pool.close()
    assert done[0] == "done" and done[1] == 7
    return out, asked, done


def test_helper_sends_its_jobs_and_handles_what_overtakes_the_reply(oracle_lib, expected, monkeypatch):
    with_batch, asked, done = _play_owner(monkeypatch, "1")
    assert len(asked) == 1 and asked[0][1:4] == (7, 10, 50) and len(asked[0][5]) == 51
    assert done[6] == expected[True]["tsv"]                              # ... and are acted on afterwards: ("opt", "want_tsv", True)
    sequential, asked0, done0 = _play_owner(monkeypatch, "0")
    assert asked0 == [] and done0[6] is None
    assert [m[0] for m in with_batch] == [m[0] for m in sequential] and with_batch[-1] == sequential[-1]
    assert with_batch[-1][2] > 0 and with_batch[-1][3] is True
    for a, b in zip(with_batch[:-1], sequential[:-1]):
        assert a[0] == "part" and a[1] == b[1] == 7 and np.array_equal(a[2], b[2])
    assert done[2:6] == done0[2:6]


def test_helper_takes_the_host_aligner_when_the_owner_cannot_run_its_jobs(oracle_lib, expected, monkeypatch):
    """("hashres", wid, None, None, None): the owner's executor failed -- the window is re-aligned in the helper, same records."""
    refused, asked, done = _play_owner(monkeypatch, "1", refuse=True)
    assert len(asked) == 1 and done[6] == expected[True]["tsv"]
    assert sum(len(m[2]) for m in refused if m[0] == "part") == refused[-1][2] == expected[True]["tsv"].count("\n")
