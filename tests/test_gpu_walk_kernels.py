"""The record kernels of the device ingest on the crafted streams of tests/walkcases.py (-m gpu): svx_bam_walk_count /
_count_seq, svx_bam_walk_extract / _extract_seq (csrc/svx_bamdev.hip) and svx_bam_walk_offsets (csrc/svx_bamindex.hip), called
through the C ABI, against the plain reference walkcases.walk_reference -- all integers, every comparison exact.

Every output lies between guard bytes of 0xA5 and is compared WITH them: a kernel that writes one byte outside what the
reference says it owns fails, also where -- in a launch over many records -- a neighbour's wave would have repaired it."""
import numpy as np
import pytest
import torch

from svision_amd import _lib, kernels
from tests import walkcases as wc

pytestmark = pytest.mark.gpu
GUARD = 64


def _dev():
    return torch.device("cuda:0")


def _raw(stream):
    """The stream at a 16-byte aligned address, at least 64 zero bytes behind it."""
    padded = np.zeros((len(stream) + 15) // 16 * 16 + 64, np.uint8)
    padded[:len(stream)] = np.frombuffer(stream, np.uint8)
    d = torch.from_numpy(padded).to(_dev())
    assert d.data_ptr() % 16 == 0
    return d


def _u64(values):
    return torch.from_numpy(np.asarray(values, np.uint64).view(np.int64).copy()).to(_dev())


class Guarded:
    """``nbytes`` of device memory, ``bias`` bytes behind a multiple of 64, pre-filled with 0xA5 like the guard bytes on both sides."""

    def __init__(self, nbytes, bias=0):
        self.at, self.n = GUARD + bias, nbytes
        self.t = torch.full((self.at + nbytes + GUARD + 64,), wc.FILL, dtype=torch.uint8, device=_dev())
        assert self.t.data_ptr() % 64 == 0
        self.ptr = self.t.data_ptr() + self.at

    def check(self, want, what):
        """The extent holds ``want`` (an array of exactly that many bytes), everything around it is untouched."""
        want = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        assert want.size == self.n, what
        expect = np.full(self.t.numel(), wc.FILL, np.uint8)
        expect[self.at:self.at + self.n] = want
        got = self.t.cpu().numpy()
        if not np.array_equal(got, expect):
            bad = np.flatnonzero(got != expect)
            raise AssertionError("%s: %d bytes differ, the first at %d of an extent of %d (guards: %d in front)" % (what, bad.size, bad[0] - self.at, self.n, self.at))


def _count(lib, d_raw, case, seq):
    """-> counts [n_starts, 4], seq_bytes [n_starts] (None without ``seq``) of one count launch, the rows around them checked."""
    n = len(case.starts) - 1
    d_starts = _u64(case.starts)
    counts, seq_bytes = Guarded(32 * n), Guarded(8 * n)
    st = kernels._stream_ptr(_dev())
    if seq:
        _lib.check(lib.svx_bam_walk_count_seq(d_raw.data_ptr(), d_starts.data_ptr(), n, counts.ptr, seq_bytes.ptr, st), "svx_bam_walk_count_seq")
    else:
        _lib.check(lib.svx_bam_walk_count(d_raw.data_ptr(), d_starts.data_ptr(), n, counts.ptr, st), "svx_bam_walk_count")
    torch.cuda.synchronize()
    got = counts.t.cpu().numpy()[counts.at:counts.at + 32 * n].view(np.int64).reshape(n, 4)
    got_seq = seq_bytes.t.cpu().numpy()[seq_bytes.at:seq_bytes.at + 8 * n].view(np.int64)
    counts.check(got, case.name + " counts")                    # (the guards around the rows)
    seq_bytes.check(got_seq if seq else np.full(8 * n, wc.FILL, np.uint8), case.name + " seq_bytes")      # (without bases: not written at all)
    return got, got_seq if seq else None


@pytest.fixture(scope="module")
def cases():
    return wc.shape_cases() + wc.cg_cases()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("seq", [False, True], ids=["count", "count_seq"])
def test_count_pass(lib, cases, seq):
    for case in cases:
        d_raw = _raw(case.stream)
        counts, seq_bytes = _count(lib, d_raw, case, seq)
        assert np.array_equal(counts, case.ref.counts), case
        assert not seq or np.array_equal(seq_bytes, case.ref.seq_bytes), case


def _bases(counts, seq_bytes):
    """Exclusive prefix sums per start, as svision_amd.ingest_gpu finish_group takes them."""
    n = counts.shape[0]
    base, seq_base = np.zeros((n, 3), np.int64), np.zeros(n, np.int64)
    if n > 1:
        base[1:] = np.cumsum(counts[:-1, :3], axis=0)
        seq_base[1:] = np.cumsum(seq_bytes[:-1])
    return base, seq_base


def _extract(lib, d_raw, d_starts, n_starts, d_base, d_seq_base, ref, seq, seq_dst=0, name_dst=0):
    """One extract launch into guarded outputs sized by the reference -> {name: (Guarded, expected)}."""
    n = len(ref.records)
    out = {"tid": (Guarded(4 * n), ref.tid), "pos": (Guarded(4 * n), ref.pos), "flag": (Guarded(2 * n), ref.flag), "mapq": (Guarded(n), ref.mapq),
           "l_seq": (Guarded(4 * n), ref.l_seq), "cig_off": (Guarded(8 * (n + 1)), ref.cig_off), "cigar": (Guarded(4 * ref.cigar.size, name_dst & ~3), ref.cigar),
           "name_off": (Guarded(8 * (n + 1)), ref.name_off), "names": (Guarded(ref.names.size, name_dst), ref.names)}
    args = [d_raw.data_ptr(), d_starts, n_starts, d_base] + [out[k][0].ptr for k in ("tid", "pos", "flag", "mapq", "l_seq", "cig_off", "cigar", "name_off", "names")]
    st = kernels._stream_ptr(_dev())
    if seq:
        out["seq_off"] = (Guarded(8 * (n + 1)), ref.seq_off)
        out["seq"] = (Guarded(ref.seq.size, seq_dst), ref.seq)
        assert out["seq"][0].ptr % 16 == seq_dst
        _lib.check(lib.svx_bam_walk_extract_seq(*args, d_seq_base, out["seq_off"][0].ptr, out["seq"][0].ptr, n, st), "svx_bam_walk_extract_seq")
    else:
        _lib.check(lib.svx_bam_walk_extract(*args, n, st), "svx_bam_walk_extract")
    return out


@pytest.mark.parametrize("seq", [False, True], ids=["extract", "extract_seq"])
def test_extract_pass(lib, cases, seq):
    """Element for element the reference's arrays -- tid / pos, which carry the records' byte offsets between the two launches,
    hold the fields afterwards --, the closing entries of the three offset arrays also where no interval has a record, and not
    a byte outside them."""
    for case in cases:
        ref = case.ref
        d_raw = _raw(case.stream)
        counts, seq_bytes = _count(lib, d_raw, case, True)
        assert np.array_equal(counts, ref.counts) and np.array_equal(seq_bytes, ref.seq_bytes), case
        base, seq_base = _bases(counts, seq_bytes)
        d_starts, d_base, d_seq_base = _u64(case.starts), _u64(base), _u64(seq_base)
        out = _extract(lib, d_raw, d_starts.data_ptr(), len(case.starts) - 1, d_base.data_ptr(), d_seq_base.data_ptr(), ref, seq)
        torch.cuda.synchronize()
        for name, (g, want) in out.items():
            g.check(want, "%s %s" % (case.name, name))


def test_walk_offsets(lib, cases):
    for case in cases:
        ref = case.ref
        d_raw = _raw(case.stream)
        base, _seq_base = _bases(ref.counts, ref.seq_bytes)
        d_starts, d_base = _u64(case.starts), _u64(base)
        rec_off = Guarded(8 * len(ref.records))
        _lib.check(lib.svx_bam_walk_offsets(d_raw.data_ptr(), d_starts.data_ptr(), len(case.starts) - 1, d_base.data_ptr(), rec_off.ptr, kernels._stream_ptr(_dev())),
                   "svx_bam_walk_offsets")
        torch.cuda.synchronize()
        rec_off.check(ref.rec_off, case.name + " rec_off")


def test_status(lib):
    """include/svx.h: 0 the chain ends on the next start, 1 it steps over it (the records are good: a stale index), 2 a record is
    malformed against the end of the part.  Only the count pass runs on these streams; rows of status 0 hold the counts."""
    for case, bad, status in wc.status_cases():
        d_raw = _raw(case.stream)
        for seq in (False, True):
            counts, seq_bytes = _count(lib, d_raw, case, seq)
            print(case.name, "status", counts[:, 3].tolist(), "reference", case.ref.counts[:, 3].tolist())
            assert counts[:, 3].tolist() == case.ref.counts[:, 3].tolist(), case
            ok = counts[:, 3] == 0
            assert np.array_equal(counts[ok], case.ref.counts[ok]), case
            assert not seq or np.array_equal(seq_bytes[ok], case.ref.seq_bytes[ok]), case
            assert bad is None or counts[bad, 3] == status, case


def test_one_record_between_guard_bytes(lib):
    """One record a launch of svx_bam_walk_extract_seq: every (SEQ source, destination) pair modulo 16 with fewer bytes than the
    head, with one chunk and with three chunks + a tail, every (CIGAR source, QNAME destination) pair modulo 4.  No neighbour
    writes next to the record: what lies in front of and behind its bytes must still be 0xA5 -- a chunk stored whole across
    the record's boundary, harmless by luck in a dense launch, is seen here."""
    guard = wc.guard_cases()
    # all streams in one buffer, each at a multiple of 64 with 64 zero bytes behind it; all outputs in one tensor per array, the
    # launches' extents 64-byte aligned + the case's bias, guards in between; one read-back per array at the end
    raw_at, out_at, at, o = [], [], 0, {k: 0 for k in ("seq", "names", "cigar")}
    for c in guard:
        raw_at.append(at)
        at += (len(c.stream) + 15) // 16 * 16 + 64
        at = (at + 63) // 64 * 64
        r = c.ref
        here = {}
        for k, nbytes, bias in (("seq", r.seq.size, c.seq_dst), ("names", r.names.size, c.name_dst), ("cigar", 4 * r.cigar.size, c.name_dst & ~3)):
            here[k] = o[k] + GUARD + bias
            o[k] = (here[k] + nbytes + GUARD + 63) // 64 * 64
        out_at.append(here)
    raw = np.zeros(at, np.uint8)
    for c, a in zip(guard, raw_at):
        raw[a:a + len(c.stream)] = np.frombuffer(c.stream, np.uint8)
    d_raw = torch.from_numpy(raw).to(_dev())
    n = len(guard)
    big = {k: torch.full((o[k] + GUARD,), wc.FILL, dtype=torch.uint8, device=_dev()) for k in o}
    # the per-record arrays: launch i owns entry 4 i + 1 (the offset arrays: 4 i + 1 and 4 i + 2), the entries around them are guards
    width = {"tid": 4, "pos": 4, "flag": 2, "mapq": 1, "l_seq": 4, "cig_off": 8, "name_off": 8, "seq_off": 8}
    small = {k: torch.full((4 * n * w + 64,), wc.FILL, dtype=torch.uint8, device=_dev()) for k, w in width.items()}
    assert d_raw.data_ptr() % 64 == 0 and all(t.data_ptr() % 64 == 0 for t in list(big.values()) + list(small.values()))
    d_starts = _u64([v for c, a in zip(guard, raw_at) for v in c.starts])       # (offsets into the case's own stream: d_raw is passed per case)
    d_zero = _u64([0, 0, 0, 0])
    st = kernels._stream_ptr(_dev())
    for i, (c, a, here) in enumerate(zip(guard, raw_at, out_at)):
        p = {k: small[k].data_ptr() + (4 * i + 1) * w for k, w in width.items()}
        _lib.check(lib.svx_bam_walk_extract_seq(d_raw.data_ptr() + a, d_starts.data_ptr() + 16 * i, 1, d_zero.data_ptr(), p["tid"], p["pos"], p["flag"], p["mapq"], p["l_seq"],
                                                p["cig_off"], big["cigar"].data_ptr() + here["cigar"], p["name_off"], big["names"].data_ptr() + here["names"],
                                                d_zero.data_ptr(), p["seq_off"], big["seq"].data_ptr() + here["seq"], 1, st), "svx_bam_walk_extract_seq")
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in list(big.items()) + list(small.items())}
    want = {k: np.full(v.size, wc.FILL, np.uint8) for k, v in got.items()}
    for i, (c, here) in enumerate(zip(guard, out_at)):
        r = c.ref
        for k, v in (("seq", r.seq), ("names", r.names), ("cigar", r.cigar)):
            b = np.ascontiguousarray(v).view(np.uint8)
            want[k][here[k]:here[k] + b.size] = b
        for k, w in width.items():
            v = getattr(r, k)
            b = np.ascontiguousarray(v).view(np.uint8)
            assert b.size == w * (2 if k.endswith("_off") else 1)
            want[k][(4 * i + 1) * w:(4 * i + 1) * w + b.size] = b
    for k in got:
        if not np.array_equal(got[k], want[k]):
            first = int(np.flatnonzero(got[k] != want[k])[0])
            if k in o:
                i = max(j for j in range(n) if out_at[j][k] - GUARD - 16 <= first)
                raise AssertionError("%s: %s, byte %d of an extent of %d bytes" % (guard[i].name, k, first - out_at[i][k], getattr(guard[i].ref, k).nbytes))
            raise AssertionError("%s: %s" % (guard[first // (4 * width[k])].name, k))
