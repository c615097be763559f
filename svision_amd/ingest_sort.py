"""A sample from an UNSORTED BAM: its records sorted on the device (``SVX_DEVICE_SORT=1``, svision_amd/cli.py).

An aligner writes its records in the order of the reads; ``samtools sort`` + ``samtools index`` of a 60 GB long-read file take far
longer than the whole run here.  Everything that takes a BAM apart without an index is on the device already (svision_amd/index.py);
what was missing is the order.  :func:`load_sample`:

  pass      the whole file in ranges, the loop of the index build (index.record_ranges): read, inflate, CRC, svx_bam_find_starts,
            svx_bam_walk_count / _extract (``with_seq``: _count_seq / _extract_seq).  Every range's records stay on the device --
            fields, CIGAR words, names, bases --; its inflated and compressed bytes are dropped with the range
  sort      ONE svx_record_sort over all records (csrc/svx_recsort.hip): by (reference, position), records without a reference
            last, ties in file order -- the order `samtools sort` keeps for a file it reads once
  gather    svx_record_gather (tid, pos, flag, mapq, l_seq), svx_record_gather_offsets + svx_record_gather_segments (CIGAR words,
            names, bases) put every array into that order
  table     the arrays the host wants come back through pinned memory, QNAME ids are taken on the SORTED names (svx_name_ids:
            first occurrence in the sorted file), and Sample.from_device scans the gathered CIGARs where they are

The whole file's packed records are resident on the device on this path -- nothing streams out before the last range is read.
The table equals, array for array, read_bam() of the same records written as a file sorted stably by that key.  A corrupt block, a
CRC mismatch, a malformed or cut chain or a device allocation that fails raises SortIngestError; no partial result is returned.

The input may also be SAM text, a pipe, or a list of BAM / SAM inputs: what an aligner writes, taken with no alignment file in
between.  The pass then has a second form, for text:

  text      a SAM file in chunks of ``range_bytes`` of text cut at line ends (io.sam.chunk_places); a path that is no regular file
            (``-``, a FIFO, /dev/fd/N) through io.sam.StreamReader, read ONCE on a thread of its own into pinned buffers.  Per chunk:
            upload, svx_sam_lines, svx_sam_pack_count, the counts read back, svx_sam_pack_extract -- the chunk's lines become the
            arrays a range of a BAM leaves (no BAM record in between, the tags are never read), and the text is dropped.  A line whose
            CIGAR is the placeholder ``<l_seq>S<n>N`` (SVX_SAM_HOST) is encoded by io.sam.encode_line; its counts and bytes go into
            the line's own slots, so the chunk's records stay in file order
  several   the header is sort_header.merge_headers over the inputs; SAM parts resolve their names against the merged dictionary (a part
            without header is fine), a BAM part's tids go through its old -> merged table; the parts follow each other in list
            order, so the stable sort leaves ties in list order, then file order.  At most one input is ``-``
  a BAM on a pipe  what ``dorado aligner`` and ``pbmm2`` write.  Refused by default (SVX_DEVICE_SORT=write takes a BAM there).
            ``pipe_bam="stream"`` / ``SVX_PIPE_BAM=stream`` (off by default: DESIGN section 9): a source of kind "bam_pipe" -- its
            header through zlib from the stream (io.sam.StreamReader.bam_header), its BGZF members in chunks of ``range_bytes``
            compressed bytes read once into pinned buffers, and the BAM pass above over index.stream_ranges, which carries a cut
            record's blocks forward where a file's pass seeks back.  Alone or one of several inputs
Gzip data that is no BAM is refused on a pipe.  A failure closes the pipe's read end, so the aligner ends with SIGPIPE; the message names
the input and the line, or the stream offset.
"""
import struct

import numpy as np

from . import textin

STAGES = ("read", "upload", "inflate", "crc", "find_starts", "walk", "lines", "pack", "concat", "sort", "gather", "read_back", "names", "scan")


class SortIngestError(ValueError):
    pass


# ---- planning (host): what svx_record_sort is asked for, and what it does with it ----
def sort_key(tid, pos, n_ref):
    """The key the records are sorted by, ascending (uint64): ((tid < 0 ? n_ref : tid) << 32) | (uint32)(pos + 1)."""
    tid, pos = np.asarray(tid, np.int64), np.asarray(pos, np.int64)
    return (np.where(tid < 0, n_ref, tid).astype(np.uint64) << np.uint64(32)) | (pos + 1).astype(np.uint64)


def pos_bits_for(lengths, max_pos=-1):
    """The significant bits of ``pos + 1``: bit_length(longest reference + 1), at least those of the largest position seen."""
    return max(1, (max([int(v) for v in lengths], default=0) + 1).bit_length(), (int(max_pos) + 1).bit_length())


def digit_plan(n_ref, pos_bits):
    """The passes of the LSD radix sort: the shift of every 8-bit digit of the packed key ((tid') << pos_bits) | (pos + 1), lowest
    first -- pos_bits + bit_length(n_ref) significant bits, at least one pass."""
    bits = int(pos_bits) + int(n_ref).bit_length()
    return [8 * p for p in range(max(1, (bits + 7) // 8))]


def packed_key(tid, pos, n_ref, pos_bits):
    """The key as the kernels pack it (uint64): sort_key with the reference moved down to bit ``pos_bits``."""
    tid, pos = np.asarray(tid, np.int64), np.asarray(pos, np.int64)
    lo = (pos + 1).astype(np.uint64) & np.uint64((1 << int(pos_bits)) - 1)
    return (np.where(tid < 0, n_ref, tid).astype(np.uint64) << np.uint64(pos_bits)) | lo


def _cat(torch, parts, pad, dev):
    """Device arrays end to end, ``pad`` zero elements behind them (what the gathers' aligned loads may touch)."""
    dtype = parts[0].dtype
    return torch.cat(list(parts) + [torch.zeros(pad, dtype=dtype, device=dev)])


def _cat_offsets(torch, parts, totals, dev):
    """Per-range CSR offsets ([n_i + 1] each, from 0) -> one [n + 1] array over the concatenated data."""
    out, at = [], 0
    for off, total in zip(parts, totals):
        out.append(off[:-1] + at)
        at += total
    out.append(torch.full((1,), at, dtype=torch.int64, device=dev))
    return torch.cat(out)


class _Source:
    """One input of :func:`load_sample`: the textin.TextInput -- its ``kind`` ("bam", "sam": text in a regular file, "pipe": text read
    once, "bam_pipe": a BAM read once), ``path`` and the ``name`` messages call it --, its own header -- ``references``, ``lengths``,
    ``text`` (a headerless SAM part: none) --, ``bam_head`` (read_bam_header's, a BAM), ``first`` (a BAM read once: where its first
    record starts, StreamReader.bam_header's) and ``remap``: a BAM part's old -> merged tid table among several inputs."""

    def __init__(self, inp, references, lengths, text, bam_head=None, first=None):
        self.input, self.kind, self.path, self.name = inp, "bam_pipe" if first is not None else inp.kind, inp.path, inp.name
        self.references, self.lengths, self.text, self.bam_head, self.first, self.remap = references, lengths, text, bam_head, first, None


def _open_source(path, alone, stream_bam=False):
    """An input opened and its header read -> _Source.  SAM text without an @SQ line is fine as one of several inputs (not ``alone``).
    ``stream_bam``: a BAM on a pipe is taken (its header read from the stream), not refused."""
    from .io import sam
    from .io.bam import read_bam_header
    try:
        inp = textin.open_input(path)
    except (sam.SamError, OSError) as exc:
        raise SortIngestError("%s: %s" % (textin.name_of(path), exc)) from None
    if inp.kind == "bam":                                       # (gzip that is no BAM too: the reader says what the file lacks)
        try:
            head = read_bam_header(path)
        except ValueError as exc:                               # (the host reader inflates in front of the header's end: a corrupt block shows here)
            raise SortIngestError(str(exc)) from None
        return _Source(inp, head.references, head.lengths, head.header_text, head)
    if inp.peek_kind == sam.STREAM_BAM and stream_bam:
        try:
            got = inp.reader.bam_header()
        except sam.BgzfStreamError as exc:
            inp.close(failed=True)
            raise SortIngestError("%s: %s" % (inp.name, exc)) from None
        return _Source(inp, got.table.references, got.table.lengths, got.table.header_text, got.table, got.first)
    refusal = {sam.STREAM_BAM: "a BAM on a pipe is not taken under SVX_DEVICE_SORT=1 -- SVX_DEVICE_SORT=write sorts it in one pass, or give "
                               "the aligner's SAM text; SVX_PIPE_BAM=stream (load_sample's pipe_bam) takes it as it arrives, a switch that "
                               "is off by default",
               sam.STREAM_GZIP: "gzip-compressed data that is no BAM -- compressed SAM is not taken: decompress it in the pipe, "
                                "`pigz -dc x.sam.gz | ... -b -`",
               sam.STREAM_EMPTY: "no input", sam.STREAM_OTHER: "neither SAM text nor a BAM"}.get(inp.peek_kind)
    if refusal is None:
        if inp.headerless and not alone:
            return _Source(inp, [], [], inp.text.decode("latin-1"))
        try:
            head = sam.parse_header(inp.text)
            return _Source(inp, head.references, head.lengths, head.text)
        except sam.SamError as exc:
            refusal = str(exc)
    inp.close(failed=True)
    raise SortIngestError("%s: %s" % (inp.name, refusal))


def _host_packed(line, tid_of):
    """A line the kernels leave to the host -> ((tid, pos, flag, mapq, l_seq), the CIGAR words (uint32), the name bytes and their
    '\\n', the 4-bit SEQ bytes) by io.sam.encode_line -- which checks the whole line, its tags too.  The words of a placeholder CIGAR
    are those of the line's first CG:B:I tag, as the BAM walk takes them; without that tag the two operations are what they say."""
    from .io import sam
    rec = sam.encode_line(line, tid_of)
    tid, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
    words = np.frombuffer(rec, "<u4", n_cig, 36 + l_name)
    for tag in line.split(b"\t")[11:]:
        if tag == b"CG:B:I" or tag.startswith(b"CG:B:I,"):
            words = np.array([int(v) for v in tag[7:].split(b",")] if len(tag) > 7 else [], np.uint32)
            break
    seq_at = 36 + l_name + 4 * n_cig
    return (tid, pos, flag, mapq, l_seq), words, rec[36:36 + l_name - 1] + b"\n", rec[seq_at:seq_at + (l_seq + 1) // 2]


class _TextPass:
    """What the chunks of one text input share: the device, the merged dictionary as the kernels' table and as the host's, the
    reader of the chunks with its pinned buffers (textin.ChunkReader), and the count of the lines the host took."""

    def __init__(self, torch, lib, kernels, dev, clock, references, with_seq):
        from . import index
        from .io import sam
        self.torch, self.kernels, self.dev, self.clock, self.with_seq = torch, kernels, dev, clock, with_seq
        self.tid_of, self.table = sam.tid_table(references), kernels.sam_ref_table(references, dev)
        self.reader, self.host_lines, self.Range = textin.ChunkReader(torch, lib, clock), 0, index.RecordRange

    def chunk(self, src, chunk):
        """A chunk of text (textin.Chunk: its bytes in pinned memory, ``line_no`` lines in front of it) -> the RecordRange of its
        records (None: no line), the text dropped."""
        from .io import sam
        torch, kernels, dev, clock, with_seq = self.torch, self.kernels, self.dev, self.clock, self.with_seq
        n, line_no = chunk.n, chunk.line_no
        d_text, d_line_off, n_lines = textin.upload_lines(torch, kernels, dev, clock, chunk)
        if n_lines == 0:
            return None
        d_status, _d_fields, d_counts = kernels.sam_pack_count(d_text, n, d_line_off, n_lines, self.table, with_seq)
        status, counts = d_status.cpu().numpy(), d_counts.cpu().numpy().astype(np.int64)
        host = {}
        if status.any():
            line_off = d_line_off[:n_lines + 1].cpu().numpy()
            bad = np.flatnonzero(status < kernels.SAM_HOST)
            if bad.size:
                i = int(bad[0])                                 # (the error is worded of the line's 11 fields: the tags are never read here)
                line = b"\t".join(textin.line_bytes(chunk.data, line_off, i).split(b"\t")[:11])
                raise SortIngestError("%s: %s" % (src.name, textin.line_refusal(line, self.tid_of, line_no + i + 1, "svx_sam_pack_count", int(status[i]))))
            for i in np.flatnonzero(status == kernels.SAM_HOST):
                try:
                    host[int(i)] = _host_packed(textin.line_bytes(chunk.data, line_off, i), self.tid_of)
                except sam.SamError as exc:
                    raise SortIngestError("%s: %s" % (src.name, exc.at(line_no + int(i) + 1))) from None
                _fields, words, name, bases = host[int(i)]
                counts[:, i] = len(words), len(name), len(bases) if with_seq else 0
            self.host_lines += len(host)
        # ---- the records' slots: the exclusive prefix of the counts, the host's lines among them
        off = np.zeros((3, n_lines + 1), np.int64)
        np.cumsum(counts, axis=1, out=off[:, 1:])
        rng = self.Range()
        rng.n_rec, rng.words, rng.name_bytes, rng.seq_bytes = n_lines, int(off[0, -1]), int(off[1, -1]), int(off[2, -1])
        out = {"d_tid": torch.empty(n_lines, dtype=torch.int32, device=dev), "d_pos": torch.empty(n_lines, dtype=torch.int32, device=dev),
               "d_l_seq": torch.empty(n_lines, dtype=torch.int32, device=dev), "d_flag": torch.empty(n_lines, dtype=torch.int16, device=dev),
               "d_mapq": torch.empty(n_lines, dtype=torch.uint8, device=dev),
               "d_cigar": torch.empty(max(rng.words, 1) + 4, dtype=torch.int32, device=dev),
               "d_names": torch.empty(max(rng.name_bytes, 1), dtype=torch.uint8, device=dev)}
        if with_seq:
            out["d_seq"] = torch.empty((max(rng.seq_bytes, 1) + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        d_off = kernels.sam_pack_extract(d_text, n, d_line_off, n_lines, self.table, d_status, list(off[:3 if with_seq else 2]), out)
        for i, (fields, words, name, bases) in host.items():
            for key, v in zip(("d_tid", "d_pos", "d_flag", "d_mapq", "d_l_seq"), fields):
                out[key][i] = v - 65536 if key == "d_flag" and v > 32767 else v
            pieces = [("d_cigar", 0, words.view(np.int32)), ("d_names", 1, np.frombuffer(name, np.uint8))]
            if with_seq:
                pieces.append(("d_seq", 2, np.frombuffer(bases, np.uint8)))
            for key, k, piece in pieces:
                if piece.size:
                    out[key][int(off[k, i]):int(off[k, i]) + piece.size].copy_(torch.from_numpy(piece.copy()))
        for key, t in out.items():
            setattr(rng, key, t)
        rng.d_cig_off, rng.d_name_off = d_off[0], d_off[1]
        if with_seq:
            rng.d_seq_off = d_off[2]
        clock.lap("pack")
        return rng

    def parts(self, src, range_bytes):
        """Generator: the RecordRange of every chunk of the text input ``src``."""
        for chunk in self.reader.chunks(src.input, range_bytes):
            yield self.chunk(src, chunk)


def _remapped(torch, src, d_tid, dev):
    """A BAM part's packed tids through its old -> merged table; -1 stays, a value outside the part's dictionary raises."""
    if bool(((d_tid < -1) | (d_tid >= len(src.remap))).any()):
        raise SortIngestError("%s: a record names a reference outside the file's dictionary of %d" % (src.name, len(src.remap)))
    if np.array_equal(src.remap, np.arange(len(src.remap))):
        return d_tid
    d_map = torch.from_numpy(np.ascontiguousarray(src.remap, np.int32)).to(dev)
    return torch.where(d_tid < 0, d_tid, d_map[d_tid.clamp(min=0).long()])


def load_sample(bam_path, fasta, min_sv, device="cuda", with_seq=False, range_bytes=None, stats=None, pipe_bam=None):
    """The :class:`svision_amd.sample.Sample` of records that come in any order (see the head of the module).  ``bam_path``: a BAM, SAM
    text, ``-`` or another path that is no regular file (text read once), or a list of those.  ``with_seq``: the table carries the
    read bases (--hash / --graph).  ``range_bytes``: compressed bytes a range of a BAM (default: the device decoder's group size),
    text bytes a chunk of SAM text (default: textin.DEFAULT_SAM_CHUNK_BYTES), compressed bytes a chunk of a BAM on a pipe (default:
    textin.DEFAULT_PIPE_BAM_BYTES); tests.  ``stats``: a dict that receives the number of ranges and records, the CIGAR words, the
    inputs' kinds, the lines the host took, the seconds per stage and, per input that was read once, its reader's bytes and waits
    (``pipes``).  ``pipe_bam``: "stream" takes a BAM on a pipe in one pass (kind "bam_pipe"); "spool", "0" or unset refuse it as before;
    None: ``SVX_PIPE_BAM`` of the environment."""
    from . import index, kernels, sort_header
    from .io import sam
    from .io.bam import AlignmentTable
    from .sample import Sample
    torch, lib, dev, clock = index.on_device("load_sample needs the GPU (svx_record_sort)", device, STAGES)
    paths = textin.input_paths(bam_path)
    try:
        stream_bam = textin.pipe_bam_setting(pipe_bam, "load_sample")
    except ValueError as exc:
        raise SortIngestError(str(exc)) from None
    label = paths[0] if len(paths) == 1 else "%s (+ %d more)" % (paths[0], len(paths) - 1)
    if paths.count("-") > 1:
        raise SortIngestError("%s is named twice: standard input is one stream" % sam.STREAM_NAME)
    fields = ("d_tid", "d_pos", "d_flag", "d_mapq", "d_l_seq")
    parts, n, words, name_bytes, seq_bytes, ranges, host_lines, sources = [], 0, 0, 0, 0, 0, 0, []
    try:
        for p in paths:
            sources.append(_open_source(p, len(paths) == 1, stream_bam))
        if len(sources) == 1:
            references, lengths, header_text = sources[0].references, sources[0].lengths, sources[0].text
            label = sources[0].name
        else:
            try:
                merged = sort_header.merge_headers([(s.name, s.text, s.references, s.lengths) for s in sources])
            except sort_header.SortWriteError as exc:
                raise SortIngestError(str(exc)) from None
            references, lengths, header_text = merged.references, merged.lengths, merged.text
            for s, table in zip(sources, merged.maps):
                s.remap = table if s.bam_head is not None else None
        n_ref = len(references)
        try:
            with torch.cuda.device(dev):
                for src in sources:
                    text_pass = None
                    if src.kind == "bam":
                        ranges_of = index.record_ranges(src.path, src.bam_head, dev, clock, range_bytes, with_seq=with_seq)
                    elif src.kind == "bam_pipe":
                        ranges_of = index.stream_ranges(textin.member_chunks(torch, src.input, range_bytes), src.bam_head, src.first, dev, clock,
                                                        with_seq=with_seq, name=src.name)
                    else:
                        text_pass = _TextPass(torch, lib, kernels, dev, clock, references, with_seq)
                        ranges_of = text_pass.parts(src, range_bytes)
                    for rng in ranges_of:
                        ranges += 1
                        if rng is None:
                            continue
                        rng.d_raw = rng.d_starts = rng.d_base = None    # the range's inflated bytes go now, not with the next range
                        if rng.n_rec:
                            if src.remap is not None:
                                rng.d_tid = _remapped(torch, src, rng.d_tid, dev)
                            parts.append(rng)
                            n, words, name_bytes, seq_bytes = n + rng.n_rec, words + rng.words, name_bytes + rng.name_bytes, seq_bytes + rng.seq_bytes
                    if text_pass is not None:
                        host_lines += text_pass.host_lines
                        del text_pass
                if n > 0xFFFFFFFF:
                    raise SortIngestError("%s: %d records -- svx_record_sort takes up to 2^32 - 1" % (label, n))
                if n == 0:
                    raise SortIngestError("%s holds no record" % label)
                arrays = _sort_and_gather(torch, kernels, dev, clock, parts, fields, n, words, n_ref, lengths, with_seq)
        except (index.IndexBuildError, textin.ReadError) as exc:
            raise SortIngestError(str(exc)) from None
        except torch.cuda.OutOfMemoryError as exc:
            raise SortIngestError("%s: the device has no room for the file's packed records -- %d records and %d CIGAR words seen so far (%s)"
                                  % (label, n, words, str(exc).split("\n")[0])) from None
    except BaseException:
        for s in sources:
            s.input.close(failed=True)
        raise
    for s in sources:
        s.input.close()
    del parts
    host, d_cigar, d_cig_off, d_pos, pos_bits = arrays
    # QNAME ids by first occurrence in the SORTED file (ingest_gpu.DeviceDecoder._make_finish is the pattern)
    names_h = np.ascontiguousarray(host["names"][:name_bytes])
    name_off = np.ascontiguousarray(host["name_off"])
    name_id = np.empty(n, np.int32)
    uniq = np.empty(max(name_bytes, 1), np.uint8)
    ub = np.zeros(1, np.uint64)
    n_unique = int(lib.svx_name_ids(names_h.ctypes.data, name_off.ctypes.data, n, name_id.ctypes.data, uniq.ctypes.data, ub.ctypes.data))
    name_list = uniq[:int(ub[0])].tobytes().decode().split("\n")[:-1] if n_unique else []
    clock.lap("names", False)
    table = AlignmentTable(references, lengths, host["tid"], host["pos"], host["flag"].view(np.uint16), host["mapq"], host["l_seq"],
                           name_id, name_list, host["cigar"][:words].view(np.uint32), host["cig_off"], header_text)
    if with_seq:
        table.seq_packed, table.seq_off = host["seq"][:seq_bytes], host["seq_off"][:n]
    sample = Sample.from_device(table, fasta, min_sv, d_cigar[:max(words, 1)], d_cig_off, d_pos)
    clock.lap("scan")
    if stats is not None:
        stats.update(ranges=ranges, records=n, cigar_words=words, pos_bits=pos_bits, passes=len(digit_plan(n_ref, pos_bits)),
                     inputs=[s.kind for s in sources], host_lines=host_lines, seconds={k: round(v, 6) for k, v in clock.times.items()},
                     pipes=[dict(name=s.name, bytes=s.input.reader.text_bytes, reader_wait_pipe_s=round(s.input.reader.wait_pipe, 6),
                                 reader_wait_buffer_s=round(s.input.reader.wait_buffer, 6)) for s in sources if s.input.reader is not None])
    return sample


def _sort_and_gather(torch, kernels, dev, clock, parts, fields, n, words, n_ref, lengths, with_seq):
    """The ranges' arrays end to end, one sort, the gathers, the host's copies -> ({name: host array}, d_cigar with 4 spare words,
    d_cig_off, d_pos, pos_bits), the device arrays in sorted order."""
    cat = {f: torch.cat([getattr(p, f) for p in parts]) for f in fields}
    cat["d_cig_off"] = _cat_offsets(torch, [p.d_cig_off for p in parts], [p.words for p in parts], dev)
    cat["d_name_off"] = _cat_offsets(torch, [p.d_name_off for p in parts], [p.name_bytes for p in parts], dev)
    cat["d_cigar"] = _cat(torch, [p.d_cigar[:p.words] for p in parts], 4, dev)
    cat["d_names"] = _cat(torch, [p.d_names[:p.name_bytes] for p in parts], 4, dev)
    if with_seq:
        cat["d_seq_off"] = _cat_offsets(torch, [p.d_seq_off for p in parts], [p.seq_bytes for p in parts], dev)
        cat["d_seq"] = _cat(torch, [p.d_seq[:p.seq_bytes] for p in parts], 16, dev)
    for p in parts:                                             # the ranges' own arrays go: one copy of the file's records stays
        for f in fields + ("d_cig_off", "d_name_off", "d_cigar", "d_names", "d_seq_off", "d_seq"):
            setattr(p, f, None)
    max_pos = int(cat["d_pos"].max())
    pos_bits = pos_bits_for(lengths, max_pos)
    clock.lap("concat")
    order = kernels.record_sort(cat["d_tid"], cat["d_pos"], n_ref, pos_bits)
    clock.lap("sort")
    out = {f[2:]: kernels.record_gather(cat[f], order) for f in fields}
    segs = [("cigar", "d_cigar", "d_cig_off", "cig_off", 4), ("names", "d_names", "d_name_off", "name_off", 4)]
    if with_seq:
        segs.append(("seq", "d_seq", "d_seq_off", "seq_off", 16))
    for name, data, off, off_name, pad in segs:
        d_off = kernels.record_gather_offsets(cat[off], order)
        total = int(cat[data].numel()) - pad
        d_out = torch.empty(total + pad, dtype=cat[data].dtype, device=dev)
        d_out[total:] = 0                                       # (the scan reads 16-byte quads: 4 readable words behind the CIGARs)
        kernels.record_gather_segments(cat[data], cat[off], order, d_off, d_out)
        out[name], out[off_name] = d_out, d_off
        cat[data] = cat[off] = None
    clock.lap("gather")
    # the host's copies through pinned memory, one event behind them all
    host = {}
    for k, d in out.items():
        h = torch.empty(int(d.numel()), dtype=d.dtype, pin_memory=True)
        h.copy_(d, non_blocking=True)
        host[k] = h
    ev = torch.cuda.Event()
    ev.record()
    ev.synchronize()
    # (copies in ordinary memory: the table outlives this call, and the helper processes of -t N are forked from this one --
    # pinned pages are not mapped into a forked child)
    host = {k: h.numpy().copy() for k, h in host.items()}
    clock.lap("read_back")
    return host, out["cigar"], out["cig_off"], out["pos"], pos_bits
