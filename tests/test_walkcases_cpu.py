"""The crafted record streams of tests/walkcases.py, without a GPU: the classes the record kernels branch on are all there
(conditions on the inputs, computed from the reference alone), the reference equals the host decoder (svx_bam.cpp, through
svision_amd.io.bam.read_bam) on every well-formed stream, the host decoder refuses every stream the reference calls malformed,
and the block table of tests/test_gpu_crc.py holds every (dst_off mod 4, len mod 4) class at both ends of the size range."""
import numpy as np
import pytest

from svision_amd.io import bam
from tests import baicases, walkcases as wc


@pytest.fixture(scope="module")
def shape():
    return wc.shape_cases()


@pytest.fixture(scope="module")
def cg():
    return wc.cg_cases()


@pytest.fixture(scope="module")
def guard():
    return wc.guard_cases()


def test_shape_cases_hold_every_class(shape):
    f = wc.facts(shape)
    assert f["n_starts"] >= set(wc.N_STARTS)
    assert f["empty_middle"] and f["empty_last"] and f["all_empty"] and f["first_start_not_0"] and f["ends_with_bases"]
    empty = next(c for c in shape if c.name == "every-interval-empty").ref
    assert not empty.records and empty.cig_off.tolist() == empty.name_off.tolist() == empty.seq_off.tolist() == [0]
    assert f["l_read_name"] >= set(wc.NAME_LENGTHS) | {0}
    assert f["cigar"] >= {(n, a) for n in wc.CIGAR_COUNTS for a in range(4)}
    assert f["l_seq"] >= set(wc.SEQ_LENGTHS)
    assert f["chunks"] >= {(c, odd) for c in wc.CHUNK_COUNTS for odd in (0, 1)}
    assert f["agree_chunks"] >= {65, 130}                       # plain 16-byte moves, more than one turn of the wave
    assert {c for c in f["agree_chunks"] if c} and f["heads"] >= set(range(16)) and f["tails"] >= set(range(16))
    assert f["lookalikes"] == 0                                 # (the placeholder's shape belongs to the CG cases)


def test_cg_cases_hold_every_class(cg):
    f = wc.facts(cg)
    case = cg[0]
    rec = case.ref.records
    assert f["cg_counts"] >= set(wc.CG_COUNTS) and f["cg_mod4"] == {0, 1, 2, 3} and f["cg_with_bases"]
    assert all(rec[k]["tagged"] for k in case.taken) and len(case.taken) == 13
    assert all(rec[k]["placeholder"] and rec[k]["n_words"] == 2 for k in case.not_taken) and f["lookalikes"] == len(case.not_taken) == 7
    # every type of 4.2.4 lies in front of one taken tag
    k = next(k for k in case.taken if rec[k]["n_words"] == 9)
    p = rec[k]["off"]
    front = case.stream[rec[k]["seq_at"]:rec[k]["cig_at"]]
    assert p < rec[k]["seq_at"] and all(b"X%s%s" % (t, t) in front for t in (b"A", b"c", b"C", b"s", b"S", b"i", b"I", b"f", b"Z", b"H"))
    assert all(b"Y%sB%s" % (s, s) in front for s in (b"c", b"C", b"s", b"S", b"i", b"I", b"f"))
    # with bases: the SEQ bytes lie behind the two placeholder words, the tag's words far behind them
    k = next(k for k in case.taken if rec[k]["l_seq"] == 77)
    assert rec[k]["seq_at"] == rec[k]["off"] + 36 + rec[k]["l_read_name"] + 8 and rec[k]["cig_at"] > rec[k]["seq_at"] + 39 + 77


def test_guard_cases_hold_every_pair(guard):
    f = wc.facts(guard)
    assert len(guard) <= 800 and all(len(c.ref.records) == 1 for c in guard)
    assert set(f["seq_pairs"]) == {(s, d) for s in range(16) for d in range(16)}
    for (s, d), kinds in f["seq_pairs"].items():
        assert kinds >= ({1, 3} if d in (0, 15) else {"short", 1, 3}), (s, d)
    assert f["tails"] == set(range(16)) and f["heads"] == set(range(16))
    assert f["cigar_name_pairs"] >= {(a, d) for a in range(4) for d in range(4)}


def test_status_cases(shape):
    cases = wc.status_cases()
    kinds = {c.name for c, _i, _s in cases}
    assert len(kinds) == len(cases) == 11
    good = next(c for c, i, _s in cases if i is None)
    assert wc.status_reference(good.stream, good.starts) == [0] * 8
    for case, bad, status in cases:
        if bad is None:
            continue
        got = wc.status_reference(case.stream, case.starts)
        assert got[bad] == status, case
        if case.starts[:bad] + case.starts[bad + 2:] == good.starts[:bad] + good.starts[bad + 2:] and case.stream == good.stream:
            # a moved start: the two intervals it borders change, no other (counts included)
            changed = [i for i in range(8) if got[i] != 0 or (case.ref.counts[i] != good.ref.counts[i]).any()]
            assert set(changed) <= {bad - 1, bad, bad + 1} and got.count(1) == 1, case
        else:
            assert [s for i, s in enumerate(got) if i != bad] == [0] * 5, case
    five = next(c for c, _i, _s in cases if c.name == "status-start-5-bytes-into-a-record")
    assert five.ref.counts[:, 3].tolist()[:3] == [0, 0, 1]     # the interval IN FRONT of the start that points into a record
    assert wc.status_reference(shape[0].stream, shape[0].starts) == [0]


def _same_as_host(case, tmp_path):
    path = str(tmp_path / (case.name + ".bam"))
    baicases.write_stream(path, wc.host_stream(case))
    t = bam.read_bam(path, with_seq=True)
    ref = case.ref
    n = len(ref.records)
    assert len(t) == n and not ref.counts[:, 3].any()
    for f in ("tid", "pos", "flag", "mapq", "l_seq"):
        assert np.array_equal(getattr(t, f), getattr(ref, f)), f
    assert np.array_equal(t.cig_off, ref.cig_off) and np.array_equal(np.asarray(t.cigar, np.uint32), ref.cigar)
    assert np.array_equal(np.asarray(t.seq_off), ref.seq_off[:n]) and bytes(t.seq_packed) == ref.seq.tobytes()
    names = ref.names.tobytes().decode().split("\n")[:-1]
    assert [t.names[i] for i in t.name_id] == names and len(names) == n
    assert int(ref.counts[:, 0].sum()) == n and int(ref.counts[:, 1].sum()) == ref.cigar.size and int(ref.counts[:, 2].sum()) == ref.names.size
    assert int(ref.seq_bytes.sum()) == ref.seq.size


def test_reference_equals_the_host_decoder(shape, cg, guard, tmp_path):
    cases = [c for c in shape + cg if c.host] + guard[::37] + [c for c, i, _s in wc.status_cases() if i is None]
    assert {c.name for c in cases} >= {"shape-1", "shape-130", "every-interval-empty", "cg", "status-good"}
    for case in cases:
        _same_as_host(case, tmp_path)


def test_an_empty_name_on_a_files_first_record(tmp_path):
    """l_read_name 1 -- nothing but the NUL -- on the first record of a file: the host decoder's name arena had no slab yet and
    took the empty name's room from none (a crash).  Found by the one-record streams of the guard cases."""
    b = wc.Builder(seed=31)
    b.add(1, 3, 20)
    b.add(9, 2, 7)
    b.add(1, 0, 0)
    case = wc.Case("empty-first-name", b.buf, [0, len(b.buf)])
    assert [r["l_read_name"] for r in case.ref.records] == [1, 9, 1]
    _same_as_host(case, tmp_path)


def test_the_host_decoder_refuses_the_malformed_streams(tmp_path):
    n = 0
    for case, bad, status in wc.status_cases():
        if status != 2:
            continue
        n += 1
        path = str(tmp_path / (case.name + ".bam"))
        baicases.write_stream(path, wc.host_stream(case))
        with pytest.raises(ValueError, match="malformed|index|truncated"):
            bam.read_bam(path, with_seq=True)
    assert n == 8


def test_crc_block_table():
    lengths = wc.crc_lengths()
    assert sorted(lengths) == wc.CRC_SHORT + wc.CRC_MIDDLE + wc.CRC_LONG and len(set(lengths)) == len(lengths)
    every = {(o, l) for o in range(4) for l in range(4)}
    assert wc.crc_classes(lengths, lambda v: 4 <= v <= 300) == every        # (below 4 bytes the kernel goes byte by byte)
    assert wc.crc_classes(lengths, lambda v: v >= 65230) == every
    assert sum(lengths) < 21 << 20
