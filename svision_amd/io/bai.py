"""The bytes of a standard ``.bai`` (SAMv1 5.2) from the records of a coordinate-sorted BAM, with htslib's conventions
(hts_idx_push / hts_idx_finish): vectorised NumPy -- a whole genome holds a few million records, which is no work for a kernel.

* ``bin = reg2bin(pos, end)`` with ``end = pos + reference span`` (``pos + 1`` where the span is 0);
* one chunk per run of records of equal (reference, bin), from the run's first record to the first record behind it;
* the pseudo-bin 37450 per reference that has records: its offset range and its mapped / unmapped counts;
* the 16 kb linear index: per window the first record overlapping it, empty windows back-filled from the right;
* ``n_no_coor``: the records without a reference, behind all others.

The records come from svision_amd.index.build_index (device record walk) -- or from anywhere else: nothing here touches a device.
"""
import numpy as np

META_BIN = 37450


def reg2bin(beg, end):
    """SAMv1 5.3 for arrays: the smallest bin that holds [beg, end)."""
    beg = np.asarray(beg, np.int64)
    last = np.asarray(end, np.int64) - 1
    out = np.zeros(beg.shape, np.int64)
    done = np.zeros(beg.shape, bool)
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        same = ~done & ((beg >> shift) == (last >> shift))
        out[same] = first + (beg[same] >> shift)
        done |= same
    return out


def virtual_offsets(dst_off, coff, off):
    """Byte offsets ``off`` into the inflated bytes of blocks that lie at the file offsets ``coff`` and inflate to
    ``dst_off[i]`` .. ``dst_off[i + 1]`` -> BGZF virtual offsets ``coff << 16 | offset in the block``.  An offset exactly behind a
    block's last byte belongs to offset 0 of the next block that holds data, or of the last block where none does."""
    coff = np.asarray(coff, np.uint64)
    starts = np.asarray(dst_off, np.uint64)[:coff.size]
    off = np.asarray(off, np.uint64)
    blk = np.searchsorted(starts, off, "right") - 1
    return (coff[blk] << np.uint64(16)) | (off - starts[blk])


def check_sorted(tid, pos):
    """ValueError unless the records are coordinate-sorted: references ascending, positions ascending inside one, the records
    without a reference last."""
    tid, pos = np.asarray(tid, np.int64), np.asarray(pos, np.int64)
    if tid.size < 2:
        return
    key = np.where(tid < 0, np.int64(1) << 40, tid)             # (no reference: behind every reference)
    down = (key[1:] < key[:-1]) | ((key[1:] == key[:-1]) & (tid[1:] >= 0) & (pos[1:] < pos[:-1]))
    if down.any():
        i = int(np.flatnonzero(down)[0]) + 1
        raise ValueError("the BAM is not coordinate-sorted: record %d (reference %d, position %d) lies behind record %d (reference %d, position %d)"
                         % (i, tid[i], pos[i], i - 1, tid[i - 1], pos[i - 1]))


class TooLong(ValueError):
    """A placed record the index format cannot address: ``tid``, ``pos``, ``end`` of the first such record in file order."""

    def __init__(self, tid, pos, end, why):
        ValueError.__init__(self, "%s: the record at position %d of reference %d ends at %d" % (why, pos, tid, end))
        self.tid, self.pos, self.end, self.why = tid, pos, end, why


LIMIT = 1 << 29                                                 # the first position the five levels over 16 kb windows cannot address


class Parts:
    """What :func:`index_parts` makes of a record list, for the writer of either format.  The placed records' ``voff`` / ``voff_end``
    and ``n_no_coor``; the chunks as runs sorted by (reference, bin, file order) -- ``run_beg`` / ``run_end`` -- in groups of one
    (reference, bin): ``grp_at`` (its first run), ``grp_n``, ``grp_tid``, ``grp_bin``, and per reference its groups [``grp_lo``,
    ``grp_hi``); per reference its records [``rec_lo``, ``rec_hi``) and the running count of unmapped ones (``unmapped``); the linear
    index of all references in one array (``linear``), reference t's ``n_intv[t]`` windows from ``lin_at[t]`` on."""


def index_parts(n_ref, tid, pos, end, flag, voff, voff_end, bin_of, window_shift=14, limit=None):
    """The checks and the grouping both index formats share -> (:class:`Parts`).  ``bin_of(pos, end)``: the format's bins;
    ``window_shift``: log2 of a linear window; ``limit``: (first position the format cannot hold, what to say then) or None."""
    tid, pos, end = np.asarray(tid, np.int64), np.asarray(pos, np.int64), np.asarray(end, np.int64)
    flag, voff, voff_end = np.asarray(flag, np.int64), np.asarray(voff, np.uint64), np.asarray(voff_end, np.uint64)
    n_ref = int(n_ref)
    if tid.size and int(tid.max()) >= n_ref:
        raise ValueError("a record names reference %d of %d" % (int(tid.max()), n_ref))
    check_sorted(tid, pos)
    placed = tid >= 0
    n_no_coor = int(tid.size - np.count_nonzero(placed))
    tid, pos, end, flag, voff, voff_end = (a[placed] for a in (tid, pos, end, flag, voff, voff_end))
    n = int(tid.size)
    end = np.maximum(end, pos + 1)
    if limit is not None and n and int(end.max()) - 1 >= limit[0]:
        i = int(np.flatnonzero(end - 1 >= limit[0])[0])
        raise TooLong(int(tid[i]), int(pos[i]), int(end[i]), limit[1])
    bins = bin_of(pos, end)

    # chunks: runs of equal (tid, bin) in file order, then grouped by (tid, bin) -- a bin's chunks stay in file order
    new_run = np.ones(n, bool)
    new_run[1:] = (tid[1:] != tid[:-1]) | (bins[1:] != bins[:-1])
    run_at = np.flatnonzero(new_run)
    run_last = (np.append(run_at[1:], n) - 1)[:run_at.size]
    run_tid, run_bin, run_beg, run_end = tid[run_at], bins[run_at], voff[run_at], voff_end[run_last]
    order = np.lexsort((np.arange(run_at.size), run_bin, run_tid))
    run_tid, run_bin, run_beg, run_end = run_tid[order], run_bin[order], run_beg[order], run_end[order]
    new_group = np.ones(run_at.size, bool)
    new_group[1:] = (run_tid[1:] != run_tid[:-1]) | (run_bin[1:] != run_bin[:-1])
    grp_at = np.flatnonzero(new_group)
    grp_n = np.diff(np.append(grp_at, run_at.size))
    grp_tid, grp_bin = run_tid[grp_at], run_bin[grp_at]
    grp_lo, grp_hi = np.searchsorted(grp_tid, np.arange(n_ref), "left"), np.searchsorted(grp_tid, np.arange(n_ref), "right")

    # per reference: its records' range (sorted: one run of the array), the mapped / unmapped counts
    rec_lo, rec_hi = np.searchsorted(tid, np.arange(n_ref), "left"), np.searchsorted(tid, np.arange(n_ref), "right")
    unmapped = np.zeros(n + 1, np.int64)
    unmapped[1:] = np.cumsum((flag & 4) != 0)

    # linear index: every (record, window it overlaps) pair in file order; the first pair of a window names its record
    w0, w1 = pos >> window_shift, (end - 1) >> window_shift
    n_intv = np.zeros(n_ref, np.int64)
    if n:
        np.maximum.at(n_intv, tid, w1 + 1)
    lin_at = np.zeros(n_ref + 1, np.int64)
    lin_at[1:] = np.cumsum(n_intv)
    per = w1 - w0 + 1
    rec_of = np.repeat(np.arange(n), per)
    pair_at = np.zeros(n + 1, np.int64)
    pair_at[1:] = np.cumsum(per)
    window = lin_at[tid[rec_of]] + w0[rec_of] + (np.arange(rec_of.size) - pair_at[rec_of])
    linear = np.zeros(int(lin_at[-1]), "<u8")
    filled = np.zeros(linear.size, bool)
    uniq, first = np.unique(window, return_index=True)
    linear[uniq] = voff[rec_of[first]]
    filled[uniq] = True
    # empty windows take the entry of the next window that has one (a reference's last window always has: no entry crosses a reference)
    src = np.where(filled, np.arange(linear.size), linear.size)
    src = np.minimum.accumulate(src[::-1])[::-1]
    linear = linear[src] if linear.size else linear

    p = Parts()
    p.n_no_coor, p.voff, p.voff_end = n_no_coor, voff, voff_end
    p.run_beg, p.run_end, p.grp_at, p.grp_n, p.grp_tid, p.grp_bin, p.grp_lo, p.grp_hi = run_beg, run_end, grp_at, grp_n, grp_tid, grp_bin, grp_lo, grp_hi
    p.rec_lo, p.rec_hi, p.unmapped, p.n_intv, p.lin_at, p.linear = rec_lo, rec_hi, unmapped, n_intv, lin_at, linear
    return p


def group_words(p, loffset=None):
    """Every group of ``p`` as little-endian 32-bit words -- bin, (``loffset``: its two words, the CSI's), n_chunk, then four words a
    chunk -> (words, grp_word: where each group's words begin, with a closing entry)."""
    head = 2 if loffset is None else 4
    n_run = int(p.run_beg.size)
    grp_word = np.zeros(p.grp_at.size + 1, np.int64)
    grp_word[1:] = np.cumsum(head + 4 * p.grp_n)
    words = np.zeros(int(grp_word[-1]), "<u4")
    lo32 = np.uint64(0xFFFFFFFF)
    words[grp_word[:-1]] = p.grp_bin.astype(np.uint32)
    if loffset is not None:
        loffset = np.asarray(loffset, np.uint64)
        words[grp_word[:-1] + 1] = (loffset & lo32).astype(np.uint32)
        words[grp_word[:-1] + 2] = (loffset >> np.uint64(32)).astype(np.uint32)
    words[grp_word[:-1] + head - 1] = p.grp_n.astype(np.uint32)
    grp_of_run = np.repeat(np.arange(p.grp_at.size), p.grp_n)
    chunk_word = grp_word[grp_of_run] + head + 4 * (np.arange(n_run) - p.grp_at[grp_of_run])
    words[chunk_word] = (p.run_beg & lo32).astype(np.uint32)
    words[chunk_word + 1] = (p.run_beg >> np.uint64(32)).astype(np.uint32)
    words[chunk_word + 2] = (p.run_end & lo32).astype(np.uint32)
    words[chunk_word + 3] = (p.run_end >> np.uint64(32)).astype(np.uint32)
    return words, grp_word


def meta_values(p, t):
    """The pseudo-bin's four values of reference ``t`` (which has records): offset range, mapped and unmapped counts."""
    n_un = int(p.unmapped[p.rec_hi[t]] - p.unmapped[p.rec_lo[t]])
    return [int(p.voff[p.rec_lo[t]]), int(p.voff_end[p.rec_hi[t] - 1]), int(p.rec_hi[t] - p.rec_lo[t]) - n_un, n_un]


def bai_bytes(n_ref, tid, pos, end, flag, voff, voff_end):
    """-> the index file's bytes.  Per record, in file order: ``tid``, ``pos``, ``end`` (exclusive reference end), ``flag``,
    ``voff`` (virtual offset of its first byte) and ``voff_end`` (of the first byte behind it = the next record's ``voff``).
    A placed record whose last base lies at 2^29 or beyond raises :class:`TooLong`: the format has no bin and no window for it."""
    n_ref = int(n_ref)
    p = index_parts(n_ref, tid, pos, end, flag, voff, voff_end, reg2bin, 14, (LIMIT, "a .bai cannot hold positions from 2^29 on"))
    words, grp_word = group_words(p)
    out = [b"BAI\x01", np.asarray([n_ref], "<i4").tobytes()]
    for t in range(n_ref):
        has = p.rec_hi[t] > p.rec_lo[t]
        out.append(np.asarray([p.grp_hi[t] - p.grp_lo[t] + (1 if has else 0)], "<i4").tobytes())
        out.append(words[grp_word[p.grp_lo[t]]:grp_word[p.grp_hi[t]]].tobytes())
        if has:
            out.append(np.asarray([META_BIN, 2], "<u4").tobytes())
            out.append(np.asarray(meta_values(p, t), "<u8").tobytes())
        out.append(np.asarray([p.n_intv[t]], "<i4").tobytes())
        out.append(p.linear[p.lin_at[t]:p.lin_at[t + 1]].tobytes())
    out.append(np.asarray([p.n_no_coor], "<u8").tobytes())
    return b"".join(out)
