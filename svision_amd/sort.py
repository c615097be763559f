"""Write the coordinate-sorted BAM of an unsorted one, and its ``.bai``, on the device: ``python -m svision_amd.sort in.bam -o out.bam``.

``SVX_DEVICE_SORT=1`` (svision_amd/ingest_sort.py) computes the order of an aligner's output and throws it away with the process.
Here the order becomes a file -- a standard BAM with a standard index that the default path, any number of ranks, a second caller
and a genome browser read --, with every record byte kept: qualities and aux tags too, which the packed tables drop.  The pass:

  pass      the whole file in ranges, the loop of the index build (index.record_ranges): read, inflate, CRC, svx_bam_find_starts, the
            walk, svx_cigar_scan for the reference spans (index._index_fields).  Kept per range: tid and pos on the device; tid, pos,
            flag, span and the records' byte offsets on the host; and the BYTES of the records that complete in the range, the slice
            [first record, exit_off) of the range's inflated stream.  CIGAR words, names and the rest of the range are dropped
  join      the slices end to end are one record stream with CSR offsets
  sort      ONE svx_record_sort, the key and the stability of SVX_DEVICE_SORT=1: (reference, position), no reference last, ties in
            file order
  output    svx_record_gather_offsets gives every sorted record its offset in the output stream.  That stream is cut every 0xFF00
            bytes whatever the records (they straddle blocks the way htslib's do) and taken in chunks of ``chunk_bytes``: the records
            that touch the chunk gathered (svx_record_gather_segments), its blocks deflated (svx_bgzf_deflate: fixed Huffman code or
            stored; ``tables="dynamic"``: svx_bgzf_deflate_dyn, the same parse under Huffman codes built per block wherever that is
            smaller), packed (svx_bgzf_pack), downloaded through pinned memory and appended to a temporary file
  header    the input's header with its @HD line set to SO:coordinate (VN kept, GO and SS dropped; no @HD: one is prepended; nothing
            else is added, no @PG line: the output is reproducible byte for byte), in blocks of its own through the same encoder; the
            first record opens a new block.  The encoder's member of an empty block is the 28-byte end-of-file marker, which closes
            the file
  index     svision_amd.io.bai.bai_bytes on the sorted fields, end = pos + max(span, 1), the virtual offsets from the records' stream
            offsets, the 0xFF00 cut and the prefix of the members' lengths; both files are renamed into place together

Device memory: the records' inflated bytes once -- or a span of them, see below -- (the stream is allocated before the pass, sized by
the sum of the BGZF members' ISIZE fields, and every range's slice is copied straight into it), one range of the pass, 8 bytes of key + 20 of sort workspace a
record, and one chunk -- ``chunk_bytes`` three times over (gathered bytes, 65,536-byte slots, packed members); with
``tables="dynamic"`` the encoder's token workspace besides, 73,440 bytes a block (svx_bgzf_deflate_dyn_ws_bytes), 1.125 times
``chunk_bytes``.  ``DEFAULT_CHUNK_BYTES`` is 1,024 blocks, 64 MB.  Compression by default is the fixed Huffman code over a greedy
parse: larger files than zlib's dynamic tables write.  ``tables="dynamic"`` (``--tables dynamic``, ``SVX_SORT_TABLES=dynamic``)
writes the same inflated bytes in a smaller file, at or below zlib level 1's size on the measured data (profiles/sort_write.txt).

A file larger than the device.  The records' bytes are what may not fit: keys, ranks and offsets are about 50 bytes a record.
``memory_bytes`` (``--memory BYTES`` with K / M / G, ``SVX_SORT_MEMORY``; default: half of the device memory that is free at the call --
the other half is for a range, its inflate workspace, keys and chunk buffers; a first guess, see profiles/sort_spans.txt) is the budget
for them.  Records that fit take the path above, unchanged.  Otherwise the order is still computed in ONE sort and only the bytes are
placed in pieces, the same two files byte for byte:

  key pass  the pass above keeping no record byte: keys on the device, fields and the records' lengths on the host, and per range its
            place in the file and the number of records it completed
  sort      the same svx_record_sort and svx_record_gather_offsets; svx_record_invert gives every input record its rank
  plan      :func:`plan_spans` cuts the output's record stream every ``max(memory_bytes // 0xFF00, 1)`` blocks -- whole blocks, so the
            0xFF00 cuts fall where they fall in one piece.  A span's buffer holds every record that touches the span whole: a record
            across an edge is placed in both neighbours' buffers, a buffer exceeds the span by less than two records
  span pass per span, the ranges that own a record of it (:func:`span_ranges`) and no others are read again: read, inflate, CRC,
            svx_bam_find_starts, the walk's counts and svx_bam_walk_offsets -- no field, CIGAR word or name is extracted, no CIGAR
            scanned -- and ONE svx_record_scatter_segments a range puts its records of the span at their output offsets in the
            span's buffer.  A nearly sorted input costs about one extra read of the file, a shuffled one a read a span.  A range that
            completes another number of records than in the key pass, or a record of another length, means the file changed:
            SortWriteError
  output    the span's buffer through the chunk loop without the gather, ``chunk_bytes`` capped at the span

A corrupt block, a CRC mismatch, a malformed or cut chain, a device allocation or a write that fails raises SortWriteError (a
ValueError); no file and no temporary is left behind.
"""
import collections
import os
import struct
import sys
import tempfile
import zlib

import numpy as np

from . import _lib

BLOCK = 0xFF00                                                  # htslib's block size: inflated bytes a BGZF block of the output
DEFAULT_CHUNK_BYTES = 1024 * BLOCK
TABLES = ("fixed", "dynamic")                                   # the encoder: svx_bgzf_deflate / svx_bgzf_deflate_dyn
STAGES = ("read", "upload", "inflate", "crc", "find_starts", "walk", "scan", "read_back", "keep", "join", "sort", "gather", "scatter", "deflate",
          "pack", "download", "write", "index")


class SortWriteError(ValueError):
    pass


# ---- the header (host) ----
def sorted_header_text(text):
    """The header text with its @HD line saying ``SO:coordinate``: VN kept (1.6 where there is none), GO and SS -- they describe the
    old order -- dropped, every other field and every other line as it is; without an @HD line one is prepended."""
    lines = text.split("\n")
    if lines and lines[0].startswith("@HD"):
        fields = lines[0].split("\t")[1:]
        vn = next((f for f in fields if f.startswith("VN:")), "VN:1.6")
        rest = [f for f in fields if f[:3] not in ("VN:", "SO:", "GO:", "SS:")]
        lines[0] = "\t".join(["@HD", vn, "SO:coordinate"] + rest)
        return "\n".join(lines)
    return "@HD\tVN:1.6\tSO:coordinate\n" + text


def _members(path):
    """Generator over the file's BGZF members, hopping from header to header: (file offset, member bytes, XLEN, ISIZE).  Raises
    SortWriteError where no whole member with a BC subfield stands."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        at = 0
        while at < size:
            f.seek(at)
            fixed = f.read(12)
            if len(fixed) < 12 or fixed[:4] != b"\x1f\x8b\x08\x04":
                raise SortWriteError("no BGZF block at file offset %d" % at)
            xlen = struct.unpack_from("<H", fixed, 10)[0]
            extra = f.read(xlen)
            bsize, q = None, 0
            while q + 4 <= len(extra):
                slen = struct.unpack_from("<H", extra, q + 2)[0]
                if extra[q:q + 2] == b"BC" and slen == 2 and q + 6 <= len(extra):
                    bsize = struct.unpack_from("<H", extra, q + 4)[0] + 1
                q += 4 + slen
            if bsize is None or bsize < 12 + xlen + 8 or at + bsize > size:
                raise SortWriteError("no whole BGZF block at file offset %d" % at)
            f.seek(at + bsize - 4)
            yield at, bsize, xlen, struct.unpack("<I", f.read(4))[0]
            at += bsize


def inflated_size(path):
    """The sum of the members' ISIZE fields: the file's inflated bytes, from its headers and footers alone."""
    return sum(isize for _at, _bsize, _xlen, isize in _members(path))


def _inflated_head(path, block_at, entry):
    """The inflated bytes of the file up to the first record: the blocks in front of file offset ``block_at`` and ``entry`` bytes of the
    block there."""
    out = bytearray()
    with open(path, "rb") as f:
        for at, bsize, xlen, _isize in _members(path):
            if at > block_at or (at == block_at and not entry):
                break
            f.seek(at + 12 + xlen)
            data = zlib.decompress(f.read(bsize - 12 - xlen - 8), -15)      # (index.first_record has inflated these blocks already)
            out += data[:entry] if at == block_at else data
    return bytes(out)


def sorted_header_bytes(head):
    """The inflated bytes in front of a BAM's first record -> the same with the text rewritten by :func:`sorted_header_text`; the
    reference dictionary behind the text is kept byte for byte."""
    if head[:4] != b"BAM\x01":
        raise SortWriteError("not a BAM header")
    l_text = struct.unpack_from("<i", head, 4)[0]
    text = head[8:8 + l_text].rstrip(b"\0").decode("latin-1")
    new = sorted_header_text(text).encode("latin-1")
    return b"BAM\x01" + struct.pack("<i", len(new)) + new + head[8 + l_text:]


# ---- the plan of a sort in spans (host, NumPy) ----
Span = collections.namedtuple("Span", "lo hi r_lo r_hi base size")


def plan_spans(off_out, memory_bytes):
    """The output's record stream [0, total), ``off_out`` [n + 1] being its records' offsets, cut into spans of
    ``max(memory_bytes // BLOCK, 1) * BLOCK`` bytes -- whole blocks, so the 0xFF00 cuts fall where they fall in one piece -> a list of
    Span(lo, hi, r_lo, r_hi, base, size): the stream bytes [lo, hi); the records [r_lo, r_hi) that touch them, by the rule of the
    chunk loop (records of no byte between two others included, those at a span's edge left out: they have nothing to place);
    ``base = off_out[r_lo]``, the stream offset of the span buffer's first byte, and the buffer's ``size``,
    off_out[r_hi] - base + 4: the records are placed whole, the first and the last may reach over the span's edges, so a buffer
    exceeds the span by less than two records (+ the 4 bytes of slack the encoder's aligned loads want).  No byte: no span."""
    off_out = np.asarray(off_out, np.int64)
    total = int(off_out[-1])
    span_bytes = max(int(memory_bytes) // BLOCK, 1) * BLOCK
    if memory_bytes >= total:                                   # (a budget that holds the stream: one span, whatever the rounding)
        span_bytes = max(total, 1)
    lo = np.arange(0, total, span_bytes, dtype=np.int64)
    hi = np.minimum(lo + span_bytes, total)
    r_lo = np.searchsorted(off_out, lo, "right") - 1
    r_hi = np.searchsorted(off_out, hi, "left")
    base = off_out[r_lo]
    size = off_out[r_hi] - base + 4
    return [Span(*(int(v) for v in s)) for s in zip(lo, hi, r_lo, r_hi, base, size)]


def span_ranges(rank, range_records, r_lo, r_hi):
    """The ranges of the pass that own at least one record of sorted rank in [r_lo, r_hi) -> their indices, ascending.  ``rank`` [n]:
    the rank of every record in file order; ``range_records``: the records every range completed, in file order (their sum is n)."""
    rank = np.asarray(rank)
    ends = np.cumsum(np.asarray(range_records, np.int64))
    hit = np.flatnonzero((rank >= r_lo) & (rank < r_hi))
    return np.unique(np.searchsorted(ends, hit, "right"))


def parse_memory(text):
    """"131072", "128K", "64M", "8G" (powers of 1,024; a trailing "B" and lower case are fine) -> bytes, at least 1."""
    t = str(text).strip().upper()
    if t.endswith("B") and len(t) > 1:
        t = t[:-1]
    scale = {"K": 1 << 10, "M": 1 << 20, "G": 1 << 30}.get(t[-1:], 1)
    digits = t[:-1] if scale > 1 else t
    if not digits.isdigit() or int(digits) * scale < 1:
        raise ValueError("a memory budget is a positive number of bytes with an optional K, M or G: %r" % (text,))
    return int(digits) * scale


# ---- the device steps ----
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


def _deflate_blocks(torch, deflate, dev, d_bytes, first, n_bytes):
    """The bytes d_bytes[first : first + n_bytes] (n_bytes > 0) cut every 0xFF00 and deflated -> (slots, member lengths, stored flags,
    dynamic flags: device tensors, the number of blocks)."""
    n = (n_bytes + BLOCK - 1) // BLOCK
    off = np.minimum(np.arange(n + 1, dtype=np.int64) * BLOCK, n_bytes) + first
    slots, member_len, stored, dynamic = deflate(d_bytes, torch.from_numpy(off).to(dev))
    return slots, member_len, stored, dynamic, n


def _download(torch, d, n_bytes):
    h = torch.empty(max(n_bytes, 1), dtype=torch.uint8, pin_memory=True)
    h[:n_bytes].copy_(d[:n_bytes], non_blocking=True)
    torch.cuda.current_stream(d.device).synchronize()
    return h[:n_bytes].numpy()


def sort_bam(bam_path, out_path, device="cuda", range_bytes=None, chunk_bytes=None, stats=None, tables="fixed", memory_bytes=None):
    """Write the records of ``bam_path`` in coordinate order to ``out_path`` and its index to ``out_path + ".bai"`` (see the head of the
    module); returns ``out_path``.  ``range_bytes``: compressed bytes a range of the pass (default: the device decoder's group size),
    ``chunk_bytes``: inflated bytes a chunk of the output (default DEFAULT_CHUNK_BYTES; whole blocks, at least one) -- tests pass small
    values.  ``tables``: "fixed" -- every block in the fixed Huffman code or stored -- or "dynamic": Huffman codes built per block where
    they are smaller; the inflated bytes and the index's records are the same.  ``memory_bytes``: the budget for the records' inflated
    bytes on the device (default: half of the device memory that is free at the call); a file whose records exceed it is written in
    spans, a pass over the input for each (see the head of the module) -- the same two files.  ``stats``: a dict that receives
    ranges, records, blocks, stored_blocks, dynamic_blocks, compressed_bytes, inflated_bytes, chunks, spans (1: in one piece),
    span_range_reads (ranges read again over all spans; 0 in one piece), range_records (the records every range of the pass
    completed), stream_bytes (the largest record buffer allocated) and the seconds per stage."""
    import torch
    from . import index, ingest_sort, kernels
    from .io import bai
    from .io.bam import read_bam_header
    if not torch.cuda.is_available():
        raise _lib.SvxError("sort_bam needs the GPU (svx_record_sort, svx_bgzf_deflate); there is no CPU fallback")
    if tables not in TABLES:
        raise ValueError("tables: %r is none of %s" % (tables, ", ".join(TABLES)))
    lib = _lib.load()
    deflate = _encoder(kernels, tables)
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    chunk_blocks = max(int(chunk_bytes or DEFAULT_CHUNK_BYTES) // BLOCK, 1)
    clock = index._Clock(torch, dev, STAGES)
    out_dir = os.path.dirname(os.path.abspath(out_path))
    tmp_bam = tmp_bai = None
    seen = room = 0                                             # inflated record bytes kept so far, and in all
    budget = None if memory_bytes is None else max(int(memory_bytes), 1)
    try:
        try:
            head = read_bam_header(bam_path)
            block_at, entry, _n_ref = index.first_record(bam_path)
            raw_head = _inflated_head(bam_path, block_at, entry)
            header = sorted_header_bytes(raw_head)
            room = inflated_size(bam_path) - len(raw_head)      # the records' bytes, by the members' ISIZE fields
        except (ValueError, TypeError, OSError, zlib.error, struct.error) as exc:
            raise SortWriteError("%s: %s" % (bam_path, exc)) from None
        if room < 0:
            raise SortWriteError("%s: its BGZF blocks hold fewer bytes than its header" % bam_path)
        n_ref = len(head.references)
        with torch.cuda.device(dev):
            if budget is None:                                  # half of what is free: the rest is for a range, its inflate workspace, keys and chunks
                budget = max(int(torch.cuda.mem_get_info(dev)[0]) // 2, 1)
            spanned = room > budget                             # the records do not fit: no byte is kept in the pass, the output is filled in spans
            # ---- pass: the record stream is allocated once, by the ISIZE sum (4 readable bytes behind it: the gather's aligned
            #      loads), and every range's slice goes straight to its place in it
            d_stream = None if spanned else torch.empty(room + 4, dtype=torch.uint8, device=dev)
            stream_bytes = 0 if spanned else int(d_stream.numel())
            host, d_keys, lens, ranges, range_records, places = [], [], [], 0, [], []
            for rng in index.record_ranges(bam_path, head, dev, clock, range_bytes):
                ranges += 1
                range_records.append(int(rng.n_rec))
                places.append(rng.place)
                if rng.n_rec:
                    tid, pos, flag, span, rec_off = index._index_fields(lib, torch, kernels, dev, rng, clock)
                    first, last = int(rec_off[0]), int(rng.exit_off)
                    if seen + last - first > room:
                        raise SortWriteError("%s: more record bytes than its BGZF blocks' ISIZE fields add up to (%d)" % (bam_path, room))
                    host.append((tid, pos, flag, span))
                    lens.append(np.diff(np.append(rec_off, np.uint64(last)).astype(np.int64)))
                    d_keys.append((rng.d_tid, rng.d_pos))
                    if not spanned:
                        d_stream[seen:seen + last - first].copy_(rng.d_raw[first:last])      # the records that complete in the range: contiguous there
                    seen += last - first
                rng.d_raw = rng.d_starts = rng.d_base = rng.d_cigar = rng.d_cig_off = rng.d_names = rng.d_name_off = None
                del rng
                clock.lap("keep")
            n = int(sum(l.size for l in lens))
            if n > 0xFFFFFFFF:
                raise SortWriteError("%s: %d records -- svx_record_sort takes up to 2^32 - 1" % (bam_path, n))
            # ---- join: CSR offsets and the keys of the one record stream
            if not spanned:
                d_stream[seen:] = 0
            off_in = np.zeros(n + 1, np.int64)
            if n:
                off_in[1:] = np.cumsum(np.concatenate(lens))
            d_off_in = torch.from_numpy(off_in).to(dev)
            if n:
                d_tid, d_pos = torch.cat([k[0] for k in d_keys]), torch.cat([k[1] for k in d_keys])
                tid, pos, flag, span = (np.concatenate([h[i] for h in host]) for i in range(4))
            else:
                d_tid = d_pos = torch.empty(0, dtype=torch.int32, device=dev)
                tid = pos = span = np.empty(0, np.int32)
                flag = np.empty(0, np.uint16)
            del d_keys, host, lens
            clock.lap("join")
            # ---- sort
            pos_bits = ingest_sort.pos_bits_for(head.lengths, int(pos.max()) if n else -1)
            if n:
                d_order = kernels.record_sort(d_tid, d_pos, n_ref, pos_bits)
                d_off_out = kernels.record_gather_offsets(d_off_in, d_order)
            else:                                                   # a header and no record: header blocks + the end-of-file marker
                d_order, d_off_out = torch.empty(0, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
            order = d_order.cpu().numpy().view(np.uint32).astype(np.int64)
            off_out = d_off_out.cpu().numpy()
            del d_tid, d_pos
            clock.lap("sort")
            # ---- output
            fd, tmp_bam = tempfile.mkstemp(prefix=os.path.basename(out_path) + ".", suffix=".tmp", dir=out_dir)
            member_lens, block_bytes, n_stored, n_dynamic, chunks, span_range_reads = [], [], 0, 0, 0, 0
            with os.fdopen(fd, "wb") as f:
                # the header's blocks and, behind them, an empty block: the end-of-file marker, kept for the end
                d_head = torch.from_numpy(np.frombuffer(header, np.uint8).copy()).to(dev)
                n_head = (len(header) + BLOCK - 1) // BLOCK
                h_off = np.minimum(np.arange(n_head + 2, dtype=np.int64) * BLOCK, len(header))
                h_off[n_head + 1] = len(header)
                slots, d_len, d_stored, d_dynamic = deflate(d_head, torch.from_numpy(h_off).to(dev))
                clock.lap("deflate")
                d_packed, d_file_off = kernels.bgzf_pack(slots, d_len, len(header) + kernels.BGZF_MEMBER_EXTRA * (n_head + 1))
                clock.lap("pack")
                m = d_len.cpu().numpy().astype(np.int64)
                packed = _download(torch, d_packed, int(m.sum()))
                eof = packed[int(m[:n_head].sum()):].tobytes()
                n_stored += int(d_stored[:n_head].sum())
                n_dynamic += int(d_dynamic[:n_head].sum())
                clock.lap("download")
                f.write(packed[:int(m[:n_head].sum())].tobytes())
                member_lens.append(m[:n_head])
                block_bytes.append(np.diff(h_off[:n_head + 1]))
                clock.lap("write", False)
                del slots, d_packed, d_head
                total = int(off_out[n])
                st = kernels._stream_ptr(dev)

                def put(d_bytes, first, n_bytes):
                    """The stream bytes d_bytes[first : first + n_bytes], whole blocks but for the stream's last: deflated, packed,
                    downloaded and appended to the file."""
                    nonlocal n_stored, n_dynamic
                    slots, d_len, d_stored, d_dynamic, nb = _deflate_blocks(torch, deflate, dev, d_bytes, first, n_bytes)
                    clock.lap("deflate")
                    d_packed, d_file_off = kernels.bgzf_pack(slots, d_len, n_bytes + kernels.BGZF_MEMBER_EXTRA * nb)
                    clock.lap("pack")
                    m = d_len.cpu().numpy().astype(np.int64)
                    if (m < 26).any():
                        raise SortWriteError("%s: svx_bgzf_deflate refused a block" % bam_path)
                    n_stored += int(d_stored.sum())
                    n_dynamic += int(d_dynamic.sum())
                    packed = _download(torch, d_packed, int(m.sum()))
                    clock.lap("download")
                    f.write(packed.tobytes())
                    member_lens.append(m)
                    block_bytes.append(np.diff(np.minimum(np.arange(nb + 1, dtype=np.int64) * BLOCK, n_bytes)))
                    clock.lap("write", False)

                if not spanned:
                    for lo in range(0, total, chunk_blocks * BLOCK):
                        hi = min(lo + chunk_blocks * BLOCK, total)
                        chunks += 1
                        # the records that touch stream bytes [lo, hi)
                        r_lo = int(np.searchsorted(off_out, lo, "right")) - 1
                        r_hi = int(np.searchsorted(off_out, hi, "left"))
                        base = int(off_out[r_lo])
                        d_rebased = d_off_out[r_lo:r_hi + 1] - base
                        d_rows = d_order[r_lo:r_hi].contiguous()
                        d_chunk = torch.empty(int(off_out[r_hi]) - base + 4, dtype=torch.uint8, device=dev)
                        _lib.check(lib.svx_record_gather_segments(d_stream.data_ptr(), d_off_in.data_ptr(), d_rows.data_ptr(), d_rebased.data_ptr(),
                                                                  d_chunk.data_ptr(), r_hi - r_lo, 1, st), "svx_record_gather_segments")
                        clock.lap("gather")
                        put(d_chunk, lo - base, hi - lo)
                        del d_chunk
                else:
                    # ---- spans: the record stream in pieces of the budget, each filled by a pass over the ranges that own its records
                    d_rank = kernels.record_invert(d_order)
                    rank = np.empty(n, np.int64)
                    rank[order] = np.arange(n, dtype=np.int64)
                    rec_base = np.concatenate([[0], np.cumsum(np.asarray(range_records, np.int64))])
                    plan = plan_spans(off_out, budget)
                    clock.lap("sort")
                    for sp in plan:
                        d_span = torch.empty(sp.size, dtype=torch.uint8, device=dev)
                        stream_bytes = max(stream_bytes, int(d_span.numel()))
                        d_status = torch.zeros(1, dtype=torch.int32, device=dev)
                        need = span_ranges(rank, range_records, sp.r_lo, sp.r_hi)
                        clock.lap("scatter")
                        for k, rng in zip(need, index.record_ranges(bam_path, head, dev, clock, places=[places[k] for k in need], extract=False)):
                            span_range_reads += 1
                            if rng.n_rec != range_records[k]:
                                raise SortWriteError("%s changed while it was sorted: %d records complete in the range at file offset %d, %d did in the "
                                                     "first pass" % (bam_path, rng.n_rec, places[k][0], range_records[k]))
                            d_src_off = torch.empty(rng.n_rec + 1, dtype=torch.int64, device=dev)
                            _lib.check(lib.svx_bam_walk_offsets(rng.d_raw.data_ptr(), rng.d_starts.data_ptr(), rng.n_starts, rng.d_base.data_ptr(),
                                                                d_src_off.data_ptr(), st), "svx_bam_walk_offsets")
                            d_src_off[rng.n_rec] = int(rng.exit_off)
                            clock.lap("walk")
                            kernels.record_scatter_segments(rng.d_raw, d_src_off, d_rank[int(rec_base[k]):int(rec_base[k + 1])], sp.r_lo, sp.r_hi,
                                                            d_off_out, sp.base, d_span, d_status)
                            clock.lap("scatter")
                            rng.d_raw = rng.d_starts = rng.d_base = None
                            del rng, d_src_off
                        if int(d_status.item()):
                            raise SortWriteError("%s changed while it was sorted: a record's length is not the one the first pass saw" % bam_path)
                        step = min(chunk_blocks * BLOCK, sp.hi - sp.lo)
                        for lo in range(sp.lo, sp.hi, step):
                            hi = min(lo + step, sp.hi)
                            chunks += 1
                            put(d_span, lo - sp.base, hi - lo)
                        del d_span
                f.write(eof)
            clock.lap("write", False)
            # ---- index: every block's file offset and where its bytes lie in the inflated file, the end-of-file block included
            member_lens = np.concatenate(member_lens + [np.asarray([len(eof)], np.int64)])
            block_bytes = np.concatenate(block_bytes + [np.zeros(1, np.int64)])
            coff = np.zeros(member_lens.size, np.uint64)
            coff[1:] = np.cumsum(member_lens[:-1])
            dst = np.zeros(block_bytes.size + 1, np.uint64)
            dst[1:] = np.cumsum(block_bytes)
            voff = bai.virtual_offsets(dst, coff, (off_out + len(header)).astype(np.uint64))
            tid, pos, flag, span = tid[order], pos[order].astype(np.int64), flag[order], span[order].astype(np.int64)
            try:
                data = bai.bai_bytes(n_ref, tid, pos, pos + np.maximum(span, 1), flag, voff[:-1], voff[1:])
            except ValueError as exc:
                raise SortWriteError("%s: %s" % (bam_path, exc)) from None
            fd, tmp_bai = tempfile.mkstemp(prefix=os.path.basename(out_path) + ".bai.", suffix=".tmp", dir=out_dir)
            with os.fdopen(fd, "wb") as f:
                f.write(data)
            for t in (tmp_bam, tmp_bai):
                os.chmod(t, 0o666 & ~index._umask())
            os.replace(tmp_bam, out_path)
            tmp_bam = None
            try:
                os.replace(tmp_bai, out_path + ".bai")
            except OSError:                                         # the pair or nothing: no sorted file without its index
                os.unlink(out_path)
                raise
            tmp_bai = None
            clock.lap("index", False)
    except index.IndexBuildError as exc:
        raise SortWriteError("%s: %s" % (bam_path, exc)) from None
    except torch.cuda.OutOfMemoryError as exc:
        raise SortWriteError("%s: the device has no room for the file's records -- %d inflated record bytes in all, %d seen so far, a budget of "
                             "%s bytes for them; a smaller one (--memory, SVX_SORT_MEMORY; sort_bam's memory_bytes) writes the file in more "
                             "spans (%s)" % (bam_path, room, seen, budget, str(exc).split("\n")[0])) from None
    except _lib.SvxError as exc:
        raise SortWriteError("%s: %s" % (bam_path, exc)) from None
    except OSError as exc:
        raise SortWriteError("%s: writing %s failed (%s)" % (bam_path, out_path, exc)) from None
    finally:
        for t in (tmp_bam, tmp_bai):
            if t is not None and os.path.exists(t):
                os.unlink(t)
    if stats is not None:
        stats.update(ranges=ranges, records=n, blocks=int(member_lens.size), stored_blocks=n_stored, dynamic_blocks=n_dynamic, chunks=chunks,
                     spans=len(plan) if spanned else 1, span_range_reads=span_range_reads, range_records=range_records, stream_bytes=stream_bytes,
                     memory_bytes=budget,
                     compressed_bytes=int(member_lens.sum()), inflated_bytes=int(dst[-1]), pos_bits=pos_bits,
                     passes=len(ingest_sort.digit_plan(n_ref, pos_bits)), seconds={k: round(v, 6) for k, v in clock.times.items()})
    return out_path


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(prog="python -m svision_amd.sort", description="Write the coordinate-sorted BAM of an unsorted one, and its .bai, on the GPU.")
    ap.add_argument("bam")
    ap.add_argument("-o", "--output", required=True, help="the sorted BAM to write (its index: OUTPUT + .bai)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--chunk-bytes", type=int, default=None, help="inflated bytes a chunk of the output (default %d)" % DEFAULT_CHUNK_BYTES)
    ap.add_argument("--tables", choices=TABLES, default=os.environ.get("SVX_SORT_TABLES") or "fixed",
                    help="the encoder's Huffman codes: fixed, or built per block where that is smaller (default: $SVX_SORT_TABLES, or fixed)")
    ap.add_argument("--memory", type=parse_memory, default=os.environ.get("SVX_SORT_MEMORY") or None, metavar="BYTES",
                    help="device memory for the records' inflated bytes, with an optional K, M or G; a file with more is written in spans, a "
                         "pass over the input for each (default: $SVX_SORT_MEMORY, or half of the device memory that is free)")
    ap.add_argument("--stats-json", default=None, help="also write the statistics to this file")
    args = ap.parse_args(argv)
    if args.tables not in TABLES:
        ap.error("SVX_SORT_TABLES=%s: fixed or dynamic" % args.tables)
    stats = {}
    try:
        path = sort_bam(args.bam, args.output, device=args.device, chunk_bytes=args.chunk_bytes, stats=stats, tables=args.tables,
                        memory_bytes=args.memory)
    except (SortWriteError, _lib.SvxError, OSError) as exc:
        print("svision_amd.sort: %s" % exc, file=sys.stderr)
        return 1
    if args.stats_json:
        with open(args.stats_json, "w") as f:
            json.dump(stats, f)
    print("%s: %d records in %d BGZF blocks (%s), %d -> %d bytes, %d range(s), %d chunk(s), %.2f s"
          % (path, stats["records"], stats["blocks"],
             "%d stored" % stats["stored_blocks"] + (", %d dynamic" % stats["dynamic_blocks"] if args.tables == "dynamic" else ""),
             stats["inflated_bytes"], stats["compressed_bytes"], stats["ranges"], stats["chunks"], sum(stats["seconds"].values())))
    if stats.get("spans", 1) > 1:
        print("%s: the records exceed the budget of %d bytes (--memory): written in %d span(s), %d range(s) read again"
              % (path, stats["memory_bytes"], stats["spans"], stats["span_range_reads"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
