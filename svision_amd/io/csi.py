"""The CSI index (CSIv1) of a coordinate-sorted BAM: its bytes from the records, its reader, and what the readers of this project
want of an index of either format (:func:`spans`).  Host, NumPy: nothing here touches a device.

A ``.bai`` is the binning scheme frozen at 16 kb windows under five levels: 2^29 positions and no more.  A CSI carries the two
numbers in its header -- ``min_shift`` (log2 of the smallest bin) and ``depth`` (levels under the root) -- and so reaches any
reference a BAM can name.  It has no linear index; per bin it keeps ``loffset``, the linear-index value at the bin's first window.

  magic "CSI\\1", min_shift i32, depth i32, l_aux i32, aux[l_aux], n_ref i32,
  per reference: n_bin i32, per bin: bin u32, loffset u64, n_chunk i32, per chunk: beg u64, end u64
  n_no_coor u64 (may be missing)                                   -- the whole file BGZF-compressed

Level ``l`` (0: the root) has 8^l bins, the first numbered (8^l - 1) / 7, each over 2^(min_shift + 3 (depth - l)) bases.  The
pseudo-bin ((1 << 3 (depth + 1)) - 1) / 7 + 1 holds a reference's offset range and its mapped / unmapped counts, as 37450 does in
a ``.bai`` (which is min_shift 14, depth 5).

No ``.csi`` written here has been compared with one written by htslib: the tests check that a reader following the
specification reaches, for any region, exactly the records that overlap it (tests/csilike.py).
"""
import struct
import zlib

import numpy as np

from . import bai

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MEMBER = 0xFF00                                                 # inflated bytes a BGZF member at the most


def first_bin(level):
    """The number of the first bin of ``level``."""
    return ((1 << 3 * level) - 1) // 7


def meta_bin(depth):
    return ((1 << 3 * (depth + 1)) - 1) // 7 + 1


def reg2bin(beg, end, min_shift=14, depth=5):
    """For arrays: the smallest bin that holds [beg, end) -- ``bai.reg2bin`` with the two numbers free."""
    beg = np.asarray(beg, np.int64)
    last = np.asarray(end, np.int64) - 1
    out = np.zeros(beg.shape, np.int64)
    done = np.zeros(beg.shape, bool)
    for level in range(depth, 0, -1):
        shift = min_shift + 3 * (depth - level)
        same = ~done & ((beg >> shift) == (last >> shift))
        out[same] = first_bin(level) + (beg[same] >> shift)
        done |= same
    return out


def bin_level(bins):
    """The level of every bin number of the array."""
    bins = np.asarray(bins, np.int64)
    level = np.zeros(bins.shape, np.int64)
    l = 1
    while bins.size and first_bin(l) <= int(bins.max()):
        level[bins >= first_bin(l)] = l
        l += 1
    return level


def bin_first_window(bins, depth):
    """The first smallest-bin window (units of 2^min_shift bases) every bin of the array covers."""
    bins = np.asarray(bins, np.int64)
    level = bin_level(bins)
    first = ((np.int64(1) << (3 * level)) - 1) // 7
    return (bins - first) << (3 * (depth - level))


def depth_for(longest_reference, min_shift=14):
    """The depth an index over a longest reference of that many bases is written with: the smallest ``d`` with
    2^(min_shift + 3 d) >= longest + 256.  That is what ``samtools index -c`` does as far as its behaviour is remembered here;
    nothing at hand confirms it.  It does not matter for validity: any depth that covers the longest reference is a valid CSI,
    and a reader takes the depth from the file."""
    need, d = int(longest_reference) + 256, 0
    while (1 << (min_shift + 3 * d)) < need:
        d += 1
    return d


def bgzf(data, level=6):
    """``data`` as BGZF members of at most 0xFF00 inflated bytes (zlib, host) + the end-of-file marker."""
    out = []
    for at in range(0, len(data), MEMBER):
        part = data[at:at + MEMBER]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        c = co.compress(part) + co.flush()
        if len(c) + 26 > 65536:                                 # (does not happen with zlib on 0xFF00 bytes; stored then)
            co = zlib.compressobj(0, zlib.DEFLATED, -15)
            c = co.compress(part) + co.flush()
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(c) + 25) + c
                   + struct.pack("<II", zlib.crc32(part) & 0xFFFFFFFF, len(part)))
    out.append(EOF_BLOCK)
    return b"".join(out)


def csi_payload(n_ref, lengths, tid, pos, end, flag, voff, voff_end, min_shift=14, depth=None):
    """The inflated bytes of :func:`csi_bytes`."""
    n_ref, min_shift = int(n_ref), int(min_shift)
    if depth is None:
        depth = depth_for(max([int(v) for v in lengths] + [0]), min_shift)
    depth = int(depth)
    cover = 1 << (min_shift + 3 * depth)
    p = bai.index_parts(n_ref, tid, pos, end, flag, voff, voff_end, lambda b, e: reg2bin(b, e, min_shift, depth), min_shift,
                        (cover, "a .csi of min_shift %d and depth %d cannot hold positions from %d on" % (min_shift, depth, cover)))
    # loffset: the linear index (the project's own: empty windows take the next entry) at the bin's first window
    loffset = p.linear[p.lin_at[p.grp_tid] + bin_first_window(p.grp_bin, depth)] if p.grp_bin.size else np.zeros(0, np.uint64)
    words, grp_word = bai.group_words(p, loffset)
    out = [b"CSI\x01", np.asarray([min_shift, depth, 0, n_ref], "<i4").tobytes()]
    for t in range(n_ref):
        has = p.rec_hi[t] > p.rec_lo[t]
        out.append(np.asarray([p.grp_hi[t] - p.grp_lo[t] + (1 if has else 0)], "<i4").tobytes())
        out.append(words[grp_word[p.grp_lo[t]]:grp_word[p.grp_hi[t]]].tobytes())
        if has:
            out.append(np.asarray([meta_bin(depth), 0, 0, 2], "<u4").tobytes())
            out.append(np.asarray(bai.meta_values(p, t), "<u8").tobytes())
    out.append(np.asarray([p.n_no_coor], "<u8").tobytes())
    return b"".join(out)


def csi_bytes(n_ref, lengths, tid, pos, end, flag, voff, voff_end, min_shift=14, depth=None):
    """-> the ``.csi`` file's bytes.  The records as for ``bai.bai_bytes`` and by its rules, with the general bin: one chunk per run
    of equal (reference, bin) in file order, the pseudo-bin per reference that has records, ``n_no_coor``; no aux bytes.  Per bin,
    ``loffset`` is the linear-index value at the bin's first 2^min_shift window: the first record overlapping that window or a later
    one.  ``lengths``: the references' lengths, which give the ``depth`` (:func:`depth_for`) where none is passed.  ValueError for
    records that are not sorted, that name a reference beyond ``n_ref``, or that end beyond 2^(min_shift + 3 depth)."""
    return bgzf(csi_payload(n_ref, lengths, tid, pos, end, flag, voff, voff_end, min_shift, depth))


# ---- reading ----------------------------------------------------------------------------------------------------------------
def gunzip_members(raw):
    """The inflated bytes of a file of one or many gzip members."""
    out, rest = [], raw
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        if not d.eof:
            raise zlib.error("the last gzip member is cut")
        rest = d.unused_data
    return b"".join(out)


class Csi:
    """A parsed ``.csi``: ``min_shift``, ``depth``, ``aux`` (bytes, kept as they are), ``n_no_coor`` (None where the file ends in front
    of it) and per reference ``bins`` -- [(bin, loffset, [(beg, end), ...]), ...] in file order, the pseudo-bin left out -- and
    ``meta``: (first offset, last offset, mapped, unmapped) or None where the reference has no pseudo-bin."""

    def __init__(self, min_shift, depth, aux):
        self.min_shift, self.depth, self.aux, self.bins, self.meta, self.n_no_coor = min_shift, depth, aux, [], [], None


def parse_csi(data, path="the index"):
    """:func:`read_csi` of the inflated bytes."""
    try:
        if data[:4] != b"CSI\x01":
            raise ValueError("%s is not a CSI index" % path)
        min_shift, depth, l_aux = struct.unpack_from("<iii", data, 4)
        if min_shift < 0 or depth < 0 or min_shift + 3 * depth > 62 or l_aux < 0 or 16 + l_aux + 4 > len(data):
            raise ValueError("%s: min_shift %d, depth %d, %d aux bytes: no CSI header" % (path, min_shift, depth, l_aux))
        csi = Csi(min_shift, depth, bytes(data[16:16 + l_aux]))
        p = 16 + l_aux
        n_ref = struct.unpack_from("<i", data, p)[0]
        p += 4
        pseudo = meta_bin(depth)
        unpack = struct.unpack_from
        for _ in range(n_ref):
            n_bin = unpack("<i", data, p)[0]
            p += 4
            bins, meta = [], None
            for _b in range(n_bin):
                bin_id, loffset, n_chunk = unpack("<IQi", data, p)
                p += 16
                if bin_id > pseudo or n_chunk < 0:
                    raise ValueError("%s: bin %d lies outside depth %d" % (path, bin_id, depth))
                vals = unpack("<%dQ" % (2 * n_chunk), data, p)
                p += 16 * n_chunk
                if bin_id == pseudo:
                    meta = tuple(vals[:4]) if n_chunk == 2 else meta
                else:
                    bins.append((bin_id, loffset, list(zip(vals[0::2], vals[1::2]))))
            csi.bins.append(bins)
            csi.meta.append(meta)
        if p + 8 <= len(data):
            csi.n_no_coor = unpack("<Q", data, p)[0]
        return csi
    except struct.error:
        raise ValueError("%s is cut: it ends inside the index" % path) from None


def read_csi(path):
    """``.csi`` -> :class:`Csi`.  Takes what other writers leave: ``loffset`` values that are lower bounds only or 0, adjacent chunks
    merged, a reference without the pseudo-bin, a file that ends in front of ``n_no_coor``, aux bytes, a container of one member or of
    many.  ValueError naming the path for a bad magic, a cut file or a bin number outside the depth."""
    with open(path, "rb") as f:
        raw = f.read()
    try:
        data = gunzip_members(raw)
    except zlib.error as exc:
        raise ValueError("%s is not a CSI index, or is cut: it does not inflate (%s)" % (path, exc)) from None
    return parse_csi(data, path)


# ---- what the readers want of an index, of either format --------------------------------------------------------------------------
def voff_at(span, coord):
    """Linear-index look-up: the virtual offset of the first record of the reference overlapping the 16 kb bin of ``coord`` or
    a later one (SAMv1 5.1.3) -- every record that reaches beyond the start of that bin lies at or behind it --, clamped to
    the reference's records [lo, hi).  Entries of 0 (bins a writer left unfilled) are skipped."""
    lo, hi, linear = span
    if coord <= 0:
        return int(lo)
    b = int(coord) >> 14
    if b >= linear.size:
        return int(hi)
    tail = linear[b:]
    nz = tail[tail != 0]
    if nz.size == 0:
        return int(hi)
    return int(min(max(int(nz[0]), int(lo)), int(hi)))


class LinearSpan(tuple):
    """A reference's records in a ``.bai``: the tuple (lo, hi, linear index) that ``read_bai_linear`` gives, with the names the device
    decoder reads an index through.  Both ends of a slice are :func:`voff_at`."""
    lo, hi, seeds = property(lambda s: s[0]), property(lambda s: s[1]), property(lambda s: s[2])
    usable = property(lambda s: s[2].size > 0)

    def from_voff(self, coord):
        return voff_at(self, coord)

    to_voff = from_voff

    def next_behind(self, coord, voff):
        """The first entry behind ``voff`` from the window of ``coord`` on, else ``hi``."""
        tail = self[2][max(0, int(coord) >> 14):]
        later = tail[tail > voff]
        return int(min(int(later[0]), int(self[1]))) if later.size else int(self[1])


class CsiSpan(tuple):
    """A reference's records in a ``.csi``: the tuple (lo, hi, seeds) -- the range of its chunks and every record start the index
    names: the chunk begins and the non-zero ``loffset`` values, ascending.

    ``from_voff(P)``: the largest ``loffset`` among the bins whose first window lies at or in front of window ``P >> min_shift``,
    else ``lo``.  The true linear index does not decrease and every ``loffset`` is a lower bound of it at its window, so every
    record that reaches beyond ``P >> min_shift << min_shift`` lies at or behind the value.
    ``to_voff(P)``: the smallest chunk begin among the bins whose interval starts at or behind ``P``, else ``hi``.  The record at
    a chunk's begin lies inside its bin, so it starts at or behind ``P``, and the file is sorted by start: every record with
    ``pos < P`` lies in front of the value."""

    def __new__(cls, bins, min_shift, depth):
        ids = np.asarray([b for b, _l, _c in bins], np.int64)
        loff = np.asarray([l for _b, l, _c in bins], np.uint64)
        has = np.asarray([len(c) > 0 for _b, _l, c in bins], bool)
        begs = np.asarray([min(x[0] for x in c) if c else 0 for _b, _l, c in bins], np.uint64)
        every = np.asarray([x[0] for _b, _l, c in bins for x in c], np.uint64)
        ends = np.asarray([x[1] for _b, _l, c in bins for x in c], np.uint64)
        lo, hi = int(every.min()), int(ends.max())
        seeds = np.unique(np.concatenate([every, loff[loff != 0]]))
        self = tuple.__new__(cls, (lo, hi, seeds))
        self.min_shift, self.depth = int(min_shift), int(depth)
        window = bin_first_window(ids, depth)
        # left ends: the bins with an loffset by first window, the running maximum of the values
        keep = loff != 0
        order = np.argsort(window[keep], kind="stable")
        self._left_window, self._left_value = window[keep][order], np.maximum.accumulate(loff[keep][order]) if keep.any() else loff[keep]
        # right ends: the bins with chunks by the start of their interval, the minimum of the first chunk begins from each on
        order = np.argsort(window[has], kind="stable")
        self._right_start = window[has][order] << self.min_shift
        self._right_value = np.minimum.accumulate(begs[has][order][::-1])[::-1]
        return self

    lo, hi, seeds = property(lambda s: s[0]), property(lambda s: s[1]), property(lambda s: s[2])
    usable = property(lambda s: s.min_shift == 14)

    def _clamp(self, v):
        return int(min(max(int(v), self[0]), self[1]))

    def from_voff(self, coord):
        if coord <= 0:
            return self[0]
        i = int(np.searchsorted(self._left_window, int(coord) >> self.min_shift, "right")) - 1
        return self[0] if i < 0 else self._clamp(self._left_value[i])

    def to_voff(self, coord):
        i = int(np.searchsorted(self._right_start, max(int(coord), 0), "left"))
        return self[1] if i >= self._right_value.size else self._clamp(self._right_value[i])

    def next_behind(self, coord, voff):
        """The first record start the index names behind ``voff``, else ``hi``."""
        i = int(np.searchsorted(self[2], np.uint64(voff), "right"))
        return int(min(int(self[2][i]), self[1])) if i < self[2].size else self[1]


def index_format(path):
    """"bai" or "csi" by the file's first bytes; ValueError naming the path for anything else."""
    with open(path, "rb") as f:
        head = f.read(1 << 16)
    if head[:4] == b"BAI\x01":
        return "bai"
    if head[:2] == b"\x1f\x8b":
        try:
            if zlib.decompressobj(31).decompress(head, 4) == b"CSI\x01":
                return "csi"
        except zlib.error:
            pass
    raise ValueError("%s is neither a BAI nor a CSI index" % path)


def spans(path, decoder=False):
    """The index ``path``, ``.bai`` or ``.csi`` by its first bytes -> per reference None (no record) or (first, last) virtual offsets
    of its records, as ``read_bai`` gives them (io.bam.read_bam, BamStream).  ``decoder``: per reference None or a
    :class:`LinearSpan` / :class:`CsiSpan` -- ``lo``, ``hi``, ``seeds``, ``from_voff(coord)``, ``to_voff(coord)``, ``usable`` --
    for ingest_gpu.DeviceDecoder."""
    from . import bam
    if index_format(path) == "bai":
        return [None if s is None else LinearSpan(s) for s in bam.read_bai_linear(path)] if decoder else bam.read_bai(path)
    csi = read_csi(path)
    out = []
    for bins in csi.bins:
        if not any(c for _b, _l, c in bins):
            out.append(None)
        elif decoder:
            out.append(CsiSpan(bins, csi.min_shift, csi.depth))
        else:
            out.append((min(x[0] for _b, _l, c in bins for x in c), max(x[1] for _b, _l, c in bins for x in c)))
    return out
