"""The output side of svision_amd/sort.py: the 0xFF00 cut, the BGZF writer and its encoder on the device, the pair of files put in
place together, and the spool file of a pipe that is not kept in core.

  output    svx_record_gather_offsets gives every sorted record its offset in the output stream.  That stream is cut every 0xFF00
            bytes whatever the records (they straddle blocks the way htslib's do) and taken in chunks of ``chunk_bytes``: the records
            that touch the chunk gathered (svx_record_gather_segments), its blocks deflated (svx_bgzf_deflate: fixed Huffman code or
            stored; ``tables="dynamic"``: svx_bgzf_deflate_dyn, the same parse under Huffman codes built per block wherever that is
            smaller), packed (svx_bgzf_pack), downloaded through pinned memory and appended to a temporary file

Device memory of a chunk: ``chunk_bytes`` three times over (gathered bytes, 65,536-byte slots, packed members); with
``tables="dynamic"`` the encoder's token workspace besides, 73,440 bytes a block (svx_bgzf_deflate_dyn_ws_bytes), 1.125 times
``chunk_bytes``.  ``DEFAULT_CHUNK_BYTES`` is 1,024 blocks, 64 MB.  Compression by default is the fixed Huffman code over a greedy
parse: larger files than zlib's dynamic tables write.  ``tables="dynamic"`` (``--tables dynamic``, ``SVX_SORT_TABLES=dynamic``)
writes the same inflated bytes in a smaller file, at or below zlib level 1's size on the measured data (profiles/sort_write.txt).

:class:`BgzfWriter` owns the temporary file and the ledger of members and is handed its encoder (:class:`DeviceEncode`; zlib in the
CPU tests); the 0xFF00 cut is one function, :func:`block_cuts`.
"""
import collections
import os

import numpy as np

from . import index
from .sort_header import SortWriteError

BLOCK = 0xFF00                                                  # htslib's block size: inflated bytes a BGZF block of the output
DEFAULT_CHUNK_BYTES = 1024 * BLOCK
STREAM_SLACK = 4                                                # readable bytes behind a record buffer: the gather's and the encoder's aligned loads

_Dev = collections.namedtuple("_Dev", "torch lib kernels dev clock")


# ---- the BGZF writer (host: the encoder is handed in) ----
def block_cuts(n_bytes, eof=False):
    """The 0xFF00 cut: ``n_bytes`` bytes in blocks of BLOCK, the last one shorter -> the blocks' offsets [blocks + 1]; ``eof``: with
    an empty block behind them."""
    n = (n_bytes + BLOCK - 1) // BLOCK + bool(eof)
    return np.minimum(np.arange(n + 1, dtype=np.int64) * BLOCK, n_bytes)


def chunk_cuts(lo, hi, step):
    """The stream bytes [lo, hi) in chunks of ``step`` -> (lo, hi) of each, in order."""
    for at in range(lo, hi, step):
        yield at, min(at + step, hi)


Written = collections.namedtuple("Written", "coff dst blocks stored_blocks dynamic_blocks chunks compressed_bytes inflated_bytes")


class BgzfWriter:
    """The output file while it is written: a temporary file beside ``path``, and the ledger of what went into it -- every member's
    length and every block's inflated bytes (what the index needs), the stored and the dynamic blocks, the chunks.

    ``encode(buffer, block offsets [n + 1]) -> (the n members end to end: host uint8 array, their lengths [n], 1 where stored, 1 where
    dynamic: host arrays)`` is all that knows how blocks are deflated and where ``buffer`` lives: :class:`DeviceEncode` in sort_bam,
    zlib over a NumPy array in tests/test_sort_steps_cpu.py.  ``clock.lap("write", False)`` closes every write.  ``source`` names the
    input in a refusal."""

    def __init__(self, path, encode, clock, source=None):
        self.encode, self.clock, self.source = encode, clock, source or path
        self.member_lens, self.block_bytes, self.stored, self.dynamic, self.chunks, self.eof = [], [], 0, 0, 0, None
        self.f, self.tmp = index.temp_beside(path)

    def _append(self, buf, first, n_bytes, eof=False):
        off = block_cuts(n_bytes, eof)
        packed, m, stored, dynamic = self.encode(buf, off + first)
        if (m < 26).any():
            raise SortWriteError("%s: svx_bgzf_deflate refused a block" % self.source)
        n = m.size - bool(eof)
        end = int(m[:n].sum())
        self.f.write(packed[:end].tobytes())
        if eof:
            self.eof = packed[end:].tobytes()
        self.stored += int(stored[:n].sum())
        self.dynamic += int(dynamic[:n].sum())
        self.member_lens.append(m[:n])
        self.block_bytes.append(np.diff(off[:n + 1]))
        self.clock.lap("write", False)

    def put_header(self, buf, n_bytes):
        """The header's bytes buf[:n_bytes] in blocks of their own -- the first record opens a new block -- and, encoded with them,
        an empty block: its member is the end-of-file marker, kept for :meth:`finish`."""
        self._append(buf, 0, n_bytes, eof=True)

    def put(self, buf, first, n_bytes):
        """A chunk: the stream bytes buf[first : first + n_bytes], whole blocks but for the stream's last, encoded and appended."""
        self._append(buf, first, n_bytes)
        self.chunks += 1

    def finish(self):
        """The end-of-file marker closes the file -> Written: every member's file offset ``coff`` and where its block's bytes lie in the
        inflated file, ``dst`` [blocks + 1], the end-of-file block included, and the counts."""
        self.f.write(self.eof)
        self.f.close()
        self.clock.lap("write", False)
        member_lens = np.concatenate(self.member_lens + [np.asarray([len(self.eof)], np.int64)])
        block_bytes = np.concatenate(self.block_bytes + [np.zeros(1, np.int64)])
        coff = np.zeros(member_lens.size, np.uint64)
        coff[1:] = np.cumsum(member_lens[:-1])
        dst = np.zeros(block_bytes.size + 1, np.uint64)
        dst[1:] = np.cumsum(block_bytes)
        return Written(coff, dst, int(member_lens.size), self.stored, self.dynamic, self.chunks, int(member_lens.sum()), int(dst[-1]))

    def discard(self):
        """The file closed and, unless it was renamed into place, removed."""
        self.f.close()
        index.discard(self.tmp)


def commit_pair(tmp_bam, out_path, bai_data, suffix=".bai"):
    """The written temporary file becomes ``out_path`` and ``bai_data`` its ``.bai`` (``suffix=".csi"``: its ``.csi``): the pair or nothing
    -- a failure leaves neither file nor temporary, a sorted file that was already in place is removed again when its index cannot follow."""
    f, tmp_bai = index.temp_beside(out_path + suffix)
    try:
        with f:
            f.write(bai_data)
        index.into_place(tmp_bam, out_path)
        try:
            index.into_place(tmp_bai, out_path + suffix)
        except OSError:
            os.unlink(out_path)
            raise
    finally:
        index.discard(tmp_bam)
        index.discard(tmp_bai)


# ---- the spool file of a pipe beyond the budget (host) ----
def spool_path(out_path, number=0):
    """The spool file of a run's pipe: beside the output; ``number``: 0 for the run's first pipe, whose name has no number."""
    return "%s.spool.%d%s.bam" % (out_path, os.getpid(), ".%d" % number if number else "")


class Spool:
    """The spool file of a pipe that is not kept in core: an UNSORTED BAM beside the output, ``out_path.spool.<pid>.bam`` -- ``header``
    (the bytes in front of a BAM's first record) and then the records as :meth:`put` is handed them, in arrival order -- written
    through :class:`BgzfWriter` and its ``encode`` (``as_buffer``: bytes -> the buffer that encoder takes).  :meth:`finish` closes it
    with the end-of-file marker and puts it in place; :meth:`discard` removes it, finished or not."""

    def __init__(self, out_path, header, encode, clock, as_buffer, source=None, number=0):
        self.path, self.bytes = spool_path(out_path, number), 0
        self.writer = BgzfWriter(self.path, encode, clock, source)
        try:
            self.writer.put_header(as_buffer(header), len(header))
        except BaseException:
            self.writer.discard()
            raise

    def put(self, buf, n_bytes, step=DEFAULT_CHUNK_BYTES):
        """The records buf[:n_bytes] (whole records; STREAM_SLACK readable bytes behind them), encoded ``step`` bytes a call."""
        for lo, hi in chunk_cuts(0, int(n_bytes), max(int(step) // BLOCK, 1) * BLOCK):
            self.writer.put(buf, lo, hi - lo)

    def finish(self):
        self.bytes = self.writer.finish().compressed_bytes
        index.into_place(self.writer.tmp, self.path)
        return self.path

    def discard(self):
        self.writer.discard()
        index.discard(self.path)


def spool_copy(reader, out_path, clock, number=0):
    """BAM on a pipe: the stream's bytes as they are -- what the reader's buffer holds, then the rest -- into the spool file
    -> (its path, the bytes); the ``spool`` stage of ``clock`` is the copy's seconds."""
    path = spool_path(out_path, number)
    f, tmp = index.temp_beside(path)
    n = 0
    try:
        with f:
            piece = bytearray(1 << 20)
            f.write(reader.buf)
            n, reader.buf = len(reader.buf), bytearray()
            while True:
                got = reader.read_into(memoryview(piece))
                if got <= 0:
                    break
                f.write(piece[:got])
                n += got
        index.into_place(tmp, path)
    finally:
        index.discard(tmp)
    clock.lap("spool", False)
    return path, n


# ---- the encoder on the device ----
def _encoder(kernels, tables):
    """-> deflate(d_in, d_in_off) -> (slots, member lengths, 1 where stored, 1 where dynamic: device tensors) of the chosen encoder."""
    if tables == "dynamic":
        def deflate(d_in, d_in_off):
            slots, member_len, btype = kernels.bgzf_deflate_dynamic(d_in, d_in_off)
            return slots, member_len, btype == 0, btype == 2
    else:
        def deflate(d_in, d_in_off):
            slots, member_len, stored = kernels.bgzf_deflate(d_in, d_in_off)
            return slots, member_len, stored, stored[:0]
    return deflate


def _download(torch, d, n_bytes):
    h = torch.empty(max(n_bytes, 1), dtype=torch.uint8, pin_memory=True)
    h[:n_bytes].copy_(d[:n_bytes], non_blocking=True)
    torch.cuda.current_stream(d.device).synchronize()
    return h[:n_bytes].numpy()


class DeviceEncode:
    """:class:`BgzfWriter`'s encoder on the device: the blocks of a device buffer deflated (``tables``), packed (svx_bgzf_pack) and
    downloaded through pinned memory, the clock lapped behind each; slots and packed members go when the call returns."""

    def __init__(self, dv, tables):
        self.dv, self.deflate = dv, _encoder(dv.kernels, tables)

    def __call__(self, d_bytes, off):
        torch, kernels, clock = self.dv.torch, self.dv.kernels, self.dv.clock
        slots, d_len, d_stored, d_dynamic = self.deflate(d_bytes, torch.from_numpy(off).to(self.dv.dev))
        clock.lap("deflate")
        d_packed, _d_file_off = kernels.bgzf_pack(slots, d_len, int(off[-1] - off[0]) + kernels.BGZF_MEMBER_EXTRA * (off.size - 1))
        clock.lap("pack")
        m = d_len.cpu().numpy().astype(np.int64)
        stored, dynamic = d_stored.cpu().numpy(), d_dynamic.cpu().numpy()
        packed = _download(torch, d_packed, int(m.sum()))
        clock.lap("download")
        return packed, m, stored, dynamic
