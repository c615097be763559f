"""Build the ``.bai`` of a BAM that has none, on the device: ``python -m svision_amd.index sample.bam [-o sample.bam.bai]`` -- or its
``.csi`` (``--csi [-m MIN_SHIFT]``), the format for references with positions from 2^29 on, which a ``.bai`` cannot address.

The device ingest engine (svision_amd/ingest_gpu.py) starts every parallel step of its record walk at an entry of the .bai
linear index; a file without one was left to the host engine.  Indexing it with the usual tools is a single-threaded pass over
the whole file.  Everything such a pass needs is on the device already -- inflate, CRC32, the record walk, the CIGAR scan that
yields every record's reference span -- except knowing where records start when nothing says so: svx_bam_find_starts
(csrc/svx_bamindex.hip) finds, per BGZF block, the first record that starts in it.  The pass:

  header     host: read_bam_header (references) + the first blocks through zlib -> where the first record starts (header_place over
             bgzf_members, the one walk of a file's members: svision_amd/sort.py takes the header's bytes and the ISIZE sum from it)
  per range  whole BGZF blocks, the decoder's group size of file a range (svx_read_range, svx_bgzf_index), then on the device
             svx_bgzf_inflate_fast -> svx_bgzf_crc32 -> svx_bam_find_starts -> svx_bam_walk_count / _extract ->
             svx_bam_walk_offsets -> svx_cigar_scan (its per-record reference span) -> tid, pos, flag, span, byte offset back
  carry      a record the range's end cuts is not lost: the next range begins with the block it starts in, and its start is
             that range's known record start -- at most one record's blocks are inflated twice.  A range in which no record
             completes is read again, twice as large
  assembly   host: svision_amd.io.bai.bai_bytes (``fmt="csi"``: io.csi.csi_bytes), written under a temporary name in the target's directory and renamed

A corrupt block, a CRC mismatch, a malformed or cut record chain or a file that is not coordinate-sorted raises IndexBuildError
(a ValueError); no file is left behind.  A plain loop: nothing here overlaps reading, inflating and walking.

The pass itself -- ranges, carry, inflate, CRC, find-starts and the walk -- is :func:`record_ranges`, a generator that leaves every
range's extracted arrays on the device; build_index adds the byte offsets and the scan per range, svision_amd/ingest_sort.py (an
UNSORTED file: its records sorted on the device) keeps the arrays and sorts them.
"""
import collections
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

from . import _lib
from .io import bai

NO_START = np.uint64(0xFFFFFFFFFFFFFFFF)                        # UINT64_MAX in d_first: no record of the chain starts in the block
STAGES = ("read", "upload", "inflate", "crc", "find_starts", "walk", "scan", "read_back", "assembly")


class IndexBuildError(ValueError):
    pass


def bgzf_members(path):
    """Generator over a file's BGZF members, hopping from header to header: (file offset, member bytes, XLEN, ISIZE).  Raises
    IndexBuildError where no whole member with a BC subfield stands."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        at = 0
        while at < size:
            f.seek(at)
            fixed = f.read(12)
            if len(fixed) < 12 or fixed[:4] != b"\x1f\x8b\x08\x04":
                raise IndexBuildError("no BGZF block at file offset %d" % at)
            xlen = struct.unpack_from("<H", fixed, 10)[0]
            extra = f.read(xlen)
            bsize, q = None, 0
            while q + 4 <= len(extra):
                slen = struct.unpack_from("<H", extra, q + 2)[0]
                if extra[q:q + 2] == b"BC" and slen == 2 and q + 6 <= len(extra):
                    bsize = struct.unpack_from("<H", extra, q + 4)[0] + 1
                q += 4 + slen
            if bsize is None or bsize < 12 + xlen + 8 or at + bsize > size:
                raise IndexBuildError("no whole BGZF block at file offset %d" % at)
            f.seek(at + bsize - 4)
            yield at, bsize, xlen, struct.unpack("<I", f.read(4))[0]
            at += bsize


HeaderPlace = collections.namedtuple("HeaderPlace", "block_at entry n_ref head isize")


def header_place(path, members=None, limit=1 << 30):
    """Host: the BAM header through zlib, block by block -> HeaderPlace(file offset of the BGZF block the first record starts in, the
    record's offset in that block's inflated bytes, number of references, the inflated bytes in front of the first record, the sum of
    the ISIZE fields of the members taken).  ``members``: a :func:`bgzf_members` of the file at its start; it is left behind the last
    member the header needed, so a caller that wants every member's ISIZE goes on where this stopped."""
    need, have, n_ref, step, isize_sum = 8, 0, None, 0, 0
    head = bytearray()
    with open(path, "rb") as f:
        for at, bsize, xlen, isize in (bgzf_members(path) if members is None else members):
            f.seek(at + 12 + xlen)
            try:
                data = zlib.decompress(f.read(bsize - 12 - xlen - 8), -15)
            except zlib.error as exc:
                raise IndexBuildError("%s: the block at file offset %d does not inflate (%s)" % (path, at, exc)) from None
            block_at, block_base = at, have
            head += data
            have += len(data)
            isize_sum += isize
            # the header's fields, as far as they are in hand: magic, l_text, text, n_ref, then per reference l_name, name, l_ref
            while have >= need:
                if step == 0:
                    if bytes(head[:4]) != b"BAM\x01":
                        raise IndexBuildError("%s is not a BAM file" % path)
                    l_text = struct.unpack_from("<i", head, 4)[0]
                    need, step = 8 + l_text + 4, 1
                elif step == 1:
                    n_ref = struct.unpack_from("<i", head, need - 4)[0]
                    left, step = n_ref, 2
                    if left:
                        need += 4
                    else:
                        step = 3
                        break
                elif step == 2:
                    l_name = struct.unpack_from("<i", head, need - 4)[0]
                    need, step = need + l_name + 4, 4
                elif step == 4:
                    left -= 1
                    if left:
                        need, step = need + 4, 2
                    else:
                        step = 3
                        break
            if step == 3:
                break
            if have > limit:
                raise IndexBuildError("%s: a BAM header of more than %d bytes" % (path, limit))
        else:
            raise IndexBuildError("%s: no BGZF block at file offset %d (the BAM header is cut)" % (path, os.path.getsize(path)))
    if need == have:                                            # the header fills its block: the first record opens the next one
        return HeaderPlace(at + bsize, 0, n_ref, bytes(head), isize_sum)
    return HeaderPlace(block_at, need - block_base, n_ref, bytes(head[:need]), isize_sum)


def first_record(path, limit=1 << 30):
    """-> (file offset of the BGZF block the first record starts in, the record's offset in that block's inflated bytes, number of
    references): :func:`header_place` without the bytes."""
    return tuple(header_place(path, limit=limit)[:3])


class _Clock:
    """Wall time per stage, the device drained at every boundary (what a stage enqueued is counted as that stage's)."""

    def __init__(self, torch, device, stages=STAGES):
        self.torch, self.device, self.t, self.times = torch, device, time.perf_counter(), dict.fromkeys(stages, 0.0)

    def lap(self, stage, device_work=True):
        if device_work:
            self.torch.cuda.synchronize(self.device)
        now = time.perf_counter()
        self.times[stage] += now - self.t
        self.t = now


def on_device(needs, device, stages=STAGES):
    """What every device routine here starts with -> (torch, libsvx, the device with its index, a :class:`_Clock` over ``stages``).
    No GPU: SvxError, ``needs`` being the caller's sentence of what it wants one for."""
    import torch
    if not torch.cuda.is_available():
        raise _lib.SvxError("%s; there is no CPU fallback" % needs)
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return torch, _lib.load(), dev, _Clock(torch, dev, stages)


def temp_beside(path):
    """A temporary file in the directory of ``path``, so that a rename puts it in place -> (the open file, its name)."""
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(os.path.abspath(path)))
    return os.fdopen(fd, "wb"), tmp


def into_place(tmp, path):
    """The closed temporary file becomes ``path``, with the mode the umask gives a new file."""
    os.chmod(tmp, 0o666 & ~_umask())
    os.replace(tmp, path)


def discard(tmp):
    if tmp is not None and os.path.exists(tmp):
        os.unlink(tmp)


def write_into_place(path, data):
    """``data`` written under a temporary name beside ``path`` and renamed; a failure leaves no file."""
    f, tmp = temp_beside(path)
    try:
        with f:
            f.write(data)
        into_place(tmp, path)
    finally:
        discard(tmp)


def _as_i64(t_np):
    return np.ascontiguousarray(t_np, np.uint64).view(np.int64)


class RecordRange:
    """One range of the file taken apart on the device (:func:`record_ranges`): its whole BGZF blocks (``blocks``, ``dst``: where each
    one's inflated bytes lie in ``d_raw``; ``total`` of them), the chain's ``exit_off`` and the records that COMPLETE in the range, in
    file order -- ``n_rec`` of them with ``words`` CIGAR words, ``name_bytes`` QNAME bytes and (``with_seq``) ``seq_bytes`` SEQ bytes --
    as the device arrays svx_bam_walk_extract(_seq) filled (None where ``n_rec`` is 0).  ``d_starts`` / ``n_starts`` / ``d_base``: what
    the walk kernels took.  ``before``: the clock's stage times when the range was begun."""
    d_tid = d_pos = d_flag = d_mapq = d_l_seq = d_cig_off = d_cigar = d_name_off = d_names = d_seq_off = d_seq = None
    d_starts = d_base = d_rec_off = None
    n_starts = n_rec = words = name_bytes = seq_bytes = 0


def _inflate_range(lib, torch, kernels, dev, pinned, blocks, entry, d_ref_len, n_ref, clock):
    """A range's blocks inflated and checked, the record starts found -> RecordRange with d_raw, dst, total, exit_off and starts.
    ``pinned``: the range's compressed bytes, or a list of host tensors that hold them end to end (:func:`stream_ranges`: the carried
    blocks, then the chunk)."""
    n, used = blocks.k, blocks.used
    st = kernels._stream_ptr(dev)
    dst = np.zeros(n + 1, np.uint64)
    dst[1:] = np.cumsum(blocks.isize.astype(np.uint64))
    total = int(dst[n])
    d_comp = torch.empty((used + 31) // 16 * 16, dtype=torch.uint8, device=dev)
    at = 0
    for piece in pinned if isinstance(pinned, (list, tuple)) else [pinned[:used]]:
        d_comp[at:at + piece.numel()].copy_(piece, non_blocking=True)
        at += piece.numel()
    d_src = torch.from_numpy(_as_i64(blocks.src_off)).to(dev)
    d_len = torch.from_numpy(np.ascontiguousarray(blocks.src_len, np.uint32).view(np.int32)).to(dev)
    d_dst = torch.from_numpy(dst.view(np.int64)).to(dev)
    clock.lap("upload")
    # (readable up to the next multiple of 16 behind its last byte: the walk's aligned loads, include/svx.h)
    d_raw = torch.empty((max(total, 1) + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
    d_status = torch.zeros(n, dtype=torch.int32, device=dev)
    d_ws = torch.empty(int(lib.svx_bgzf_inflate_fast_ws_bytes(total, n)), dtype=torch.uint8, device=dev)
    _lib.check(lib.svx_bgzf_inflate_fast(d_comp.data_ptr(), d_src.data_ptr(), d_len.data_ptr(), d_dst.data_ptr(), n, total, d_raw.data_ptr(),
                                         d_status.data_ptr(), d_ws.data_ptr(), int(d_ws.numel()), st), "svx_bgzf_inflate_fast")
    clock.lap("inflate")
    _lib.check(lib.svx_bgzf_crc32(d_raw.data_ptr(), d_dst.data_ptr(), d_comp.data_ptr(), d_src.data_ptr(), d_len.data_ptr(), n,
                                  d_status.data_ptr(), st), "svx_bgzf_crc32")
    status = d_status.cpu().numpy()
    clock.lap("crc")
    del d_ws
    if status.any():
        b = int(np.flatnonzero(status)[0])
        raise IndexBuildError("the BGZF block at file offset %d %s" % (int(blocks.coff[b]), "fails its CRC32" if status[b] == kernels.INFLATE_BAD_CRC
                                                                         else "is corrupt (inflate status %d)" % status[b]))
    # where records start: per block the first start of the chain from `entry`
    d_first = torch.empty(n, dtype=torch.int64, device=dev)
    d_exit = torch.zeros(2, dtype=torch.int64, device=dev)
    d_fws = torch.empty(int(lib.svx_bam_find_starts_ws_bytes(n)), dtype=torch.uint8, device=dev)
    _lib.check(lib.svx_bam_find_starts(d_raw.data_ptr(), d_dst.data_ptr(), n, int(entry), n_ref, d_ref_len.data_ptr(), d_first.data_ptr(),
                                       d_exit.data_ptr(), d_fws.data_ptr(), int(d_fws.numel()), st), "svx_bam_find_starts")
    first = d_first.cpu().numpy().view(np.uint64)
    exit_off, chain_status = (int(v) for v in d_exit.cpu().numpy().view(np.uint64))
    clock.lap("find_starts")
    if chain_status:
        at = min(max(int(np.searchsorted(dst[:n], np.uint64(exit_off), "right")) - 1, 0), n - 1)
        raise IndexBuildError("a malformed record %d bytes into the BGZF block at file offset %d" % (exit_off - int(dst[at]), int(blocks.coff[at])))
    rng = RecordRange()
    rng.blocks, rng.dst, rng.total, rng.exit_off, rng.d_raw = blocks, dst, total, exit_off, d_raw
    rng.starts = np.unique(np.append(first[first != NO_START], np.uint64(exit_off)))
    return rng


def _walk_range(lib, torch, kernels, dev, rng, with_seq, clock, extract=True):
    """The existing walk over a range's starts: counts -> prefix sums -> the records' fields, CIGAR words, names and (``with_seq``)
    bases, all left on the device.  ``extract=False``: the counts and prefix sums alone -- ``n_rec``, ``d_starts``, ``n_starts`` and
    ``d_base``, what svx_bam_walk_offsets takes; no field, CIGAR word or name is extracted."""
    starts, d_raw = rng.starts, rng.d_raw
    n_starts = int(starts.size) - 1
    if n_starts <= 0:
        return
    st = kernels._stream_ptr(dev)
    d_starts = torch.from_numpy(starts.view(np.int64)).to(dev)
    d_counts = torch.empty((n_starts, 4), dtype=torch.int64, device=dev)
    if with_seq:
        d_seq_counts = torch.empty(n_starts, dtype=torch.int64, device=dev)
        _lib.check(lib.svx_bam_walk_count_seq(d_raw.data_ptr(), d_starts.data_ptr(), n_starts, d_counts.data_ptr(), d_seq_counts.data_ptr(), st),
                   "svx_bam_walk_count_seq")
    else:
        _lib.check(lib.svx_bam_walk_count(d_raw.data_ptr(), d_starts.data_ptr(), n_starts, d_counts.data_ptr(), st), "svx_bam_walk_count")
    counts = d_counts.cpu().numpy()
    if counts[:, 3].any():
        i = int(np.flatnonzero(counts[:, 3])[0])
        raise IndexBuildError("the record walk from byte %d of the range's inflated stream ended with status %d" % (int(starts[i]), int(counts[i, 3])))
    base = np.zeros((n_starts, 3), np.int64)
    base[1:] = np.cumsum(counts[:-1, :3], axis=0)
    n_rec, words, name_bytes = (int(v) for v in counts[:, :3].sum(axis=0))
    if n_rec == 0:
        clock.lap("walk")
        return
    d_base = torch.from_numpy(base).to(dev)
    rng.d_starts, rng.n_starts, rng.d_base = d_starts, n_starts, d_base
    rng.n_rec, rng.words, rng.name_bytes = n_rec, words, name_bytes
    if not extract:
        clock.lap("walk")
        return
    d_tid, d_pos, d_l_seq = (torch.empty(n_rec, dtype=torch.int32, device=dev) for _ in range(3))
    d_flag, d_mapq = torch.empty(n_rec, dtype=torch.int16, device=dev), torch.empty(n_rec, dtype=torch.uint8, device=dev)
    d_cig_off, d_name_off = (torch.empty(n_rec + 1, dtype=torch.int64, device=dev) for _ in range(2))
    d_cigar = torch.empty(max(words, 1) + 4, dtype=torch.int32, device=dev)
    d_names = torch.empty(max(name_bytes, 1), dtype=torch.uint8, device=dev)
    if with_seq:
        seq_counts = d_seq_counts.cpu().numpy()
        seq_base = np.zeros(n_starts, np.int64)
        seq_base[1:] = np.cumsum(seq_counts[:-1])
        rng.seq_bytes = int(seq_counts.sum())
        d_seq_base = torch.from_numpy(seq_base).to(dev)
        rng.d_seq_off = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
        rng.d_seq = torch.empty((max(rng.seq_bytes, 1) + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        _lib.check(lib.svx_bam_walk_extract_seq(d_raw.data_ptr(), d_starts.data_ptr(), n_starts, d_base.data_ptr(), d_tid.data_ptr(), d_pos.data_ptr(),
                                                d_flag.data_ptr(), d_mapq.data_ptr(), d_l_seq.data_ptr(), d_cig_off.data_ptr(), d_cigar.data_ptr(),
                                                d_name_off.data_ptr(), d_names.data_ptr(), d_seq_base.data_ptr(), rng.d_seq_off.data_ptr(),
                                                rng.d_seq.data_ptr(), n_rec, st), "svx_bam_walk_extract_seq")
    else:
        _lib.check(lib.svx_bam_walk_extract(d_raw.data_ptr(), d_starts.data_ptr(), n_starts, d_base.data_ptr(), d_tid.data_ptr(), d_pos.data_ptr(),
                                            d_flag.data_ptr(), d_mapq.data_ptr(), d_l_seq.data_ptr(), d_cig_off.data_ptr(), d_cigar.data_ptr(),
                                            d_name_off.data_ptr(), d_names.data_ptr(), n_rec, st), "svx_bam_walk_extract")
    rng.d_tid, rng.d_pos, rng.d_flag, rng.d_mapq, rng.d_l_seq = d_tid, d_pos, d_flag, d_mapq, d_l_seq
    rng.d_cig_off, rng.d_cigar, rng.d_name_off, rng.d_names = d_cig_off, d_cigar, d_name_off, d_names
    clock.lap("walk")


def record_ranges(bam_path, head, dev, clock, range_bytes=None, with_seq=False, places=None, extract=True, first=None):
    """Generator: the whole file in ranges of about ``range_bytes`` compressed bytes (default: the device decoder's group size), each
    read, inflated, CRC-checked and walked on the device -> one :class:`RecordRange` a range, whose records are those that complete
    in it; a record the range's end cuts opens the next range, a range in which none completes is read again, twice as large.  The
    last range has ``at_end`` set.  The pass of :func:`build_index` and of svision_amd.ingest_sort.load_sample.  Raises
    IndexBuildError for a corrupt block, a CRC mismatch, a malformed chain or a file cut inside a record.  ``head``: read_bam_header's.

    Every range carries its ``place`` (file offset, compressed bytes asked for, entry offset).  ``places``: a list of such places of
    an earlier pass over the same file -- those ranges again and no others, in the list's order (svision_amd/sort.py reads the ranges
    a span of its output needs); a place that no longer gives a range raises IndexBuildError.  ``extract=False``: the walk stops at its
    counts (:func:`_walk_range`): ``n_rec`` and what svx_bam_walk_offsets takes, no fields, CIGAR words or names.  ``first``: what
    :func:`first_record` gives for the file, where the caller has it already."""
    import torch
    from . import ingest, ingest_gpu, kernels
    lib = _lib.load()
    base_bytes = int(range_bytes or ingest_gpu.LARGE_GROUP_BYTES)
    file_at, entry, n_ref = first or first_record(bam_path)
    if n_ref != len(head.references):
        raise IndexBuildError("%s: the header names %d references, its dictionary %d" % (bam_path, len(head.references), n_ref))
    size = os.path.getsize(bam_path)
    d_ref_len = torch.from_numpy(np.asarray(list(head.lengths) + [0], np.int32)).to(dev)
    want_bytes = base_bytes
    pinned = None                                               # a range's file bytes: read into pinned memory, reused from range to range
    threads = ingest.decode_threads()
    places = None if places is None else iter(places)
    clock.lap("read", False)
    while True:
        if places is not None:
            place = next(places, None)
            if place is None:
                return
            file_at, want_bytes, entry = place
        want = int(min(want_bytes, size - file_at))
        if want <= 0:
            raise IndexBuildError("%s ends without a whole BGZF block behind file offset %d" % (bam_path, file_at))
        if pinned is None or pinned.numel() < want:
            pinned = torch.empty(want, dtype=torch.uint8, pin_memory=True)
        before = dict(clock.times)
        if lib.svx_read_range(bam_path.encode(), file_at, want, pinned.data_ptr(), threads) != 0:
            raise IndexBuildError(lib.svx_bam_error().decode())
        blocks = ingest_gpu._index_blocks(lib, pinned.data_ptr(), want, file_at)
        at_end = file_at + want == size
        if blocks.k < 0 or (blocks.k == 0 and at_end) or (at_end and blocks.used != want):
            raise IndexBuildError("%s: no whole BGZF block at file offset %d" % (bam_path, file_at + max(blocks.used, 0)))
        clock.lap("read", False)
        if blocks.k == 0:
            if places is not None:
                raise IndexBuildError("%s: no whole BGZF block at file offset %d, where an earlier pass read a range" % (bam_path, file_at))
            want_bytes *= 2
            continue
        rng = _inflate_range(lib, torch, kernels, dev, pinned, blocks, entry, d_ref_len, n_ref, clock)
        exit_off, total = rng.exit_off, rng.total
        if exit_off == entry and not at_end and exit_off < total:
            if places is not None:
                raise IndexBuildError("%s: no record completes in the range at file offset %d, where an earlier pass found some" % (bam_path, file_at))
            want_bytes *= 2                                     # no record completes in the range: the same place again, twice as large
            continue
        _walk_range(lib, torch, kernels, dev, rng, with_seq, clock, extract)
        rng.before, rng.at_end, rng.place = before, at_end, (file_at, want_bytes, entry)
        if at_end and exit_off != total:
            raise IndexBuildError("%s is cut inside a record: its last record starts %d bytes before the end of the data and does not fit"
                                  % (bam_path, total - exit_off))
        yield rng
        if places is not None:
            continue
        if at_end:
            return
        want_bytes = base_bytes
        if exit_off >= total:
            file_at, entry = file_at + blocks.used, 0
        else:                                                   # the block the cut record starts in opens the next range
            b = int(np.searchsorted(rng.dst[:blocks.k], np.uint64(exit_off), "right")) - 1
            file_at, entry = int(blocks.coff[b]), exit_off - int(rng.dst[b])


def range_work(head, n_ref, dev, clock, with_seq=False, extract=True):
    """The device work of one range of :func:`stream_ranges` -> ``work(pieces, blocks, entry)``: the compressed bytes -- host uint8
    arrays that lie end to end --, their block table and the chain's entry offset through :func:`_inflate_range` and
    :func:`_walk_range` -> the RecordRange: ``exit_off``, ``total``, ``dst`` and the records that complete."""
    import torch
    from . import kernels
    lib = _lib.load()
    d_ref_len = torch.from_numpy(np.asarray(list(head.lengths) + [0], np.int32)).to(dev)

    def work(pieces, blocks, entry):
        rng = _inflate_range(lib, torch, kernels, dev, [torch.from_numpy(p) for p in pieces], blocks, entry, d_ref_len, n_ref, clock)
        if rng.exit_off != entry:                               # (no record completes: nothing to walk, as in record_ranges)
            _walk_range(lib, torch, kernels, dev, rng, with_seq, clock, extract)
        return rng
    return work


def _carried(pieces, blocks, range_at, b):
    """The compressed blocks of a range from block ``b`` on, copied out of ``pieces`` -> (their bytes as one array of its own, their
    block table with the payloads' offsets counted from that array's first byte)."""
    cut = int(blocks.coff[b]) - range_at
    out, at = np.empty(blocks.used - cut, np.uint8), 0
    for piece in pieces:
        skip = min(cut, piece.size)
        out[at:at + piece.size - skip] = piece[skip:]
        at, cut = at + piece.size - skip, cut - skip
    return out, type(blocks)(blocks.k - b, blocks.src_off[b:] - np.uint64(blocks.used - out.size), blocks.src_len[b:], blocks.isize[b:],
                             blocks.coff[b:], out.size)


def stream_ranges(chunks, head, first, dev=None, clock=None, with_seq=False, extract=True, work=None, name="the stream", stats=None):
    """:func:`record_ranges` for a BAM that is seen ONCE.  ``chunks``: the stream from the member its first record starts in on, as
    (buffer, n_bytes, stream offset) of whole BGZF members each -- io.sam.StreamReader.member_chunks; a buffer is this generator's
    until it asks for the next chunk.  ``first``: (that member's stream offset, the record's offset in its inflated bytes, the number
    of references), with ``head`` what StreamReader.bam_header gave.  -> one :class:`RecordRange` a range, whose records are those that
    complete in it, in stream order; ``at_end`` is set on the last one -- a range is therefore handed on when the chunk behind it
    has arrived, or the stream's end --; ``place``: (the stream offset of the range's first byte, its compressed bytes, the entry
    offset), for messages: no place of a stream can be read again.

    What a file's pass does by seeking is done by carrying.  A record the range's end cuts (``exit_off < total``): the compressed
    blocks from the one it starts in on are copied out of the chunk's buffer before the next chunk is asked for; they open the next
    range, ``entry`` the record's offset in the first of them -- at most one record's blocks are inflated twice.  A range in which no
    record completes is that case with every block carried: the next chunk extends it, nothing is read twice and nothing is lost --
    but every carried block is inflated again with each chunk that extends the range: growth by a chunk where the file road doubles.
    At the default chunk a record is far smaller than a chunk and this never repeats; at a small ``range_bytes`` under long reads the
    inflate work is quadratic in the record's blocks, and "inflated twice" above does not hold.
    The host holds one chunk and one carried record's blocks (``stats``: ``held_peak``, the largest sum of the two; ``carry_peak``;
    ``grown``: the ranges that completed no record; ``ranges``), besides the reader's buffers.

    ``work(pieces, blocks, entry)``: the per-range device work (default :func:`range_work` over ``dev`` and ``clock``: inflate, CRC,
    find-starts, the walk) -- handed in, the carrying runs without a device (tests/test_pipe_bam_cpu.py).  Raises IndexBuildError as
    :func:`record_ranges` does for the same bytes as a file, its words with the stream offset where those have the file offset."""
    from . import ingest_gpu
    from .io import sam
    lib = _lib.load()
    expect, entry, n_ref = first
    if n_ref != len(head.references):
        raise IndexBuildError("%s: the header names %d references, its dictionary %d" % (name, len(head.references), n_ref))
    if work is None:
        work = range_work(head, n_ref, dev, clock, with_seq, extract)
    lap = (lambda: None) if clock is None else (lambda: clock.lap("read", False))
    carry = carry_blocks = pending = None
    counts = dict(held_peak=0, carry_peak=0, grown=0, ranges=0)
    chunks = iter(chunks)
    try:
        lap()
        for buf, n, at in chunks:
            if pending is not None:
                yield pending
                pending = None
            before = None if clock is None else dict(clock.times)
            if at != expect:
                raise IndexBuildError("%s: a chunk at stream offset %d where the one at %d was due" % (name, at, expect))
            expect = at + n
            data = np.frombuffer(buf, np.uint8)[:n]
            blocks = ingest_gpu._index_blocks(lib, data.ctypes.data, n, at)
            if blocks.k <= 0 or blocks.used != n:
                raise IndexBuildError("%s: no whole BGZF block at stream offset %d" % (name, at + max(blocks.used, 0)))
            lap()
            pieces = [data]
            if carry is not None:                               # the carried blocks open the range: the chunk's payloads lie behind them
                pieces = [carry, data]
                blocks = type(blocks)(carry_blocks.k + blocks.k, *(np.concatenate([a, b]) for a, b in
                                      ((carry_blocks.src_off, blocks.src_off + np.uint64(carry.size)), (carry_blocks.src_len, blocks.src_len),
                                       (carry_blocks.isize, blocks.isize), (carry_blocks.coff, blocks.coff))), carry.size + n)
            range_at = int(blocks.coff[0])
            counts["held_peak"], counts["ranges"] = max(counts["held_peak"], blocks.used), counts["ranges"] + 1
            rng = work(pieces, blocks, entry)
            exit_off, total = int(rng.exit_off), int(rng.total)
            grown = exit_off == entry and exit_off < total      # no record completes: the range goes on with the next chunk
            if not grown:
                rng.before, rng.at_end, rng.place = before, False, (range_at, blocks.used, entry)
                pending = rng
            counts["grown"] += grown
            carry = carry_blocks = None
            entry = 0
            if exit_off < total:                                # the block the cut record starts in, and all behind it, are kept
                b = int(np.searchsorted(rng.dst[:blocks.k], np.uint64(exit_off), "right")) - 1
                carry, carry_blocks = _carried(pieces, blocks, range_at, b)
                entry = exit_off - int(rng.dst[b])
                counts["carry_peak"] = max(counts["carry_peak"], carry.size)
            del data, pieces, rng, buf
        if not counts["ranges"]:
            raise IndexBuildError("%s ends without a whole BGZF block behind stream offset %d" % (name, expect))
        if carry is not None:
            raise IndexBuildError("%s is cut inside a record: its last record starts %d bytes before the end of the data and does not fit"
                                  % (name, total - exit_off))
        if pending is not None:
            pending.at_end = True
            yield pending
    except sam.BgzfStreamError as exc:
        raise IndexBuildError("%s: %s" % (name, exc)) from None
    except IndexBuildError as exc:
        raise IndexBuildError(str(exc).replace("file offset", "stream offset")) from None
    finally:
        if stats is not None:
            stats.update(counts)
        if hasattr(chunks, "close"):
            chunks.close()


def walk_offsets(lib, torch, kernels, dev, rng, closed=False):
    """svx_bam_walk_offsets: the byte offset of every record of the range in its inflated stream, on the device [n_rec]; ``closed``:
    [n_rec + 1], the chain's ``exit_off`` behind them -- CSR offsets of the records' bytes."""
    d_off = torch.empty(rng.n_rec + (1 if closed else 0), dtype=torch.int64, device=dev)
    _lib.check(lib.svx_bam_walk_offsets(rng.d_raw.data_ptr(), rng.d_starts.data_ptr(), rng.n_starts, rng.d_base.data_ptr(), d_off.data_ptr(),
                                        kernels._stream_ptr(dev)), "svx_bam_walk_offsets")
    if closed:
        d_off[rng.n_rec] = int(rng.exit_off)
    return d_off


def _index_fields(lib, torch, kernels, dev, rng, clock):
    """What the index wants of a range's records -> host arrays tid, pos, flag, reference span, byte offset in the range's stream."""
    if rng.n_rec == 0:
        return np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, np.uint16), np.empty(0, np.int32), np.empty(0, np.uint64)
    d_rec_off = rng.d_rec_off = walk_offsets(lib, torch, kernels, dev, rng)       # (kept with the range: svision_amd/sort.py rewrites records at them)
    clock.lap("walk")
    # the reference span of every record: the scan's statistics (a CG-tag record: of its real CIGAR); no gap is long enough to be listed
    scan = kernels.cigar_scan(rng.d_cigar, rng.d_cig_off, rng.d_pos, 0x7FFFFFFF, n_words=rng.words)
    clock.lap("scan")
    out = (rng.d_tid.cpu().numpy(), rng.d_pos.cpu().numpy(), rng.d_flag.cpu().numpy().view(np.uint16), scan.stats[:, 0].contiguous().cpu().numpy(),
           d_rec_off.cpu().numpy().view(np.uint64))
    clock.lap("read_back")
    return out


FORMATS = ("bai", "csi")


def too_long_message(exc, references, switch):
    """What a caller says of a bai.TooLong: the reference's name, the position, why, and the ``switch`` that writes a .csi."""
    name = references[exc.tid] if 0 <= exc.tid < len(references) else "#%d" % exc.tid
    return "a record at position %d of %s ends at %d: %s -- %s" % (exc.pos, name, exc.end, exc.why, switch)


def index_bytes(fmt, min_shift, head, tid, pos, end, flag, voff, voff_end):
    """The assembly call of either format over the same record arrays -> the index file's bytes."""
    if fmt == "csi":
        from .io import csi
        return csi.csi_bytes(len(head.references), head.lengths, tid, pos, end, flag, voff, voff_end, min_shift=min_shift)
    return bai.bai_bytes(len(head.references), tid, pos, end, flag, voff, voff_end)


def build_index(bam_path, out_path=None, device="cuda", range_bytes=None, stats=None, fmt="bai", min_shift=14):
    """Write the ``.bai`` of ``bam_path`` to ``out_path`` (default ``bam_path + ".bai"``) and return that path; ``fmt="csi"``: its
    ``.csi`` (default ``bam_path + ".csi"``) with bins of 2^``min_shift`` bases at the lowest level.  A ``.bai`` is refused
    (IndexBuildError, no file) for a record that reaches position 2^29: there is no automatic switch of format.  ``range_bytes``:
    compressed bytes a range (default: the device decoder's group size; tests).  ``stats``: a dict that receives the number of
    ranges, blocks and records and the seconds per stage -- in total ("seconds") and per range ("per_range")."""
    from . import kernels
    from .io.bam import read_bam_header
    torch, lib, dev, clock = on_device("build_index needs the GPU (svx_bam_find_starts)", device)
    if fmt not in FORMATS:
        raise ValueError("fmt: %r is none of %s" % (fmt, ", ".join(FORMATS)))
    out_path = out_path or bam_path + "." + fmt
    head = read_bam_header(bam_path)
    parts, per_range, n_blocks, end_voff = [], [], 0, None
    for rng in record_ranges(bam_path, head, dev, clock, range_bytes):
        blocks, dst = rng.blocks, rng.dst
        tid, pos, flag, span, rec_off = _index_fields(lib, torch, kernels, dev, rng, clock)
        n_blocks += blocks.k
        parts.append((tid, pos, flag, span, bai.virtual_offsets(dst, blocks.coff, rec_off)))
        clock.lap("assembly", False)
        per_range.append(dict({k: round(clock.times[k] - rng.before[k], 6) for k in STAGES}, blocks=int(blocks.k), records=int(tid.size),
                              compressed_bytes=int(blocks.used), inflated_bytes=rng.total))
        if rng.at_end:
            end_voff = bai.virtual_offsets(dst, blocks.coff, [rng.total])
    tid, pos, flag, span, voff = (np.concatenate([p[i] for p in parts]) for i in range(5))
    voff_end = np.append(voff[1:], end_voff).astype(np.uint64)
    pos64 = pos.astype(np.int64)
    try:
        data = index_bytes(fmt, min_shift, head, tid, pos64, pos64 + np.maximum(span.astype(np.int64), 1), flag, voff, voff_end)
    except bai.TooLong as exc:
        raise IndexBuildError("%s: %s" % (bam_path, too_long_message(exc, head.references, "write a .csi instead: --csi (SVX_BUILD_INDEX=csi)"
                                                                     if fmt == "bai" else "a larger depth is needed"))) from None
    except ValueError as exc:
        raise IndexBuildError("%s: %s" % (bam_path, exc)) from None
    write_into_place(out_path, data)
    clock.lap("assembly", False)
    if stats is not None:
        stats.update(ranges=len(per_range), blocks=n_blocks, records=int(tid.size), seconds={k: round(v, 6) for k, v in clock.times.items()},
                     per_range=per_range)
    return out_path


def _umask():
    mask = os.umask(0)
    os.umask(mask)
    return mask


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m svision_amd.index", description="Build the .bai, or the .csi, of a coordinate-sorted BAM on the GPU.")
    ap.add_argument("bam")
    ap.add_argument("-o", "--output", default=None, help="the index to write (default: BAM + .bai, with --csi BAM + .csi)")
    ap.add_argument("-c", "--csi", action="store_true", help="write a .csi: the format for references with positions from 2^29 on")
    ap.add_argument("-m", "--min-shift", type=int, default=14, metavar="MIN_SHIFT", help="with --csi: log2 of the smallest bin (default 14)")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    stats = {}
    try:
        path = build_index(args.bam, args.output, device=args.device, stats=stats, **(dict(fmt="csi", min_shift=args.min_shift) if args.csi else {}))
    except (IndexBuildError, OSError) as exc:
        print("svision_amd.index: %s" % exc, file=sys.stderr)
        return 1
    print("%s: %d records in %d BGZF blocks, %d range(s), %.2f s" % (path, stats["records"], stats["blocks"], stats["ranges"],
                                                                   sum(stats["seconds"].values())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
