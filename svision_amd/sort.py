"""Write the coordinate-sorted BAM of an unsorted one -- or of SAM text --, and its ``.bai``, on the device: ``python -m svision_amd.sort in.bam -o out.bam``.

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
            (``index_format="csi"`` / ``--csi`` / ``SVX_SORT_INDEX=csi``: io.csi.csi_bytes and ``.csi``; a record that reaches position
            2^29 is refused under the default ``.bai``, and neither file is left)

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

SAM text.  An aligner's output that was never converted (minimap2, winnowmap, ngmlr, pbmm2 without --sort) is taken as it is: a file
whose first byte is ``@``, or whose first line has at least 11 tab-separated fields.  Only the front end differs -- how the records'
bytes, keys and fields come about -- and the two files are those of the same records stored as an unsorted BAM, byte for byte:

  open      the ``@`` lines are the header's text, the reference dictionary comes from @SQ SN / LN (io/sam.py); ``room`` is not known yet
  key pass  the text in chunks of ``range_bytes`` (DEFAULT_SAM_CHUNK_BYTES, 64 MB: of 16, 64 and 256 MB the fastest, profiles/sort_sam.txt)
            cut at line ends, a longer line growing its chunk: read (svx_read_range into pinned memory), upload, svx_sam_lines,
            svx_sam_measure -- a wave a line: the record's bytes or a code, tid pos flag span --, read back.  An error code raises with
            the file's line number, worded by io/sam.py.  A line the kernels leave to the host (SVX_SAM_HOST: more than 65,535 CIGAR
            operations, an ``f`` value outside the exact fast path) is encoded by io.sam.encode_line at once, its bytes kept on the host
            and its length, key and fields patched in.  Behind the pass ``room`` is exact and ``spanned`` is decided
  in one piece  the text is read a second time -- from the page cache for any file that fits the device -- and svx_sam_encode writes
            every chunk's records straight into the resident stream; the host's encodings are copied to their offsets
  in spans  the places of :func:`span_ranges` are chunks of text: each is encoded into a chunk-local buffer and goes through
            svx_record_scatter_segments like a BAM's range.  A chunk with another number of lines, or a line whose record has another
            length than in the key pass, means the file changed: SortWriteError
A regular file of compressed SAM (gzip, BGZF) is not taken: the text of a file is read twice, and there is no device decoder for it.

A pipe.  ``minimap2 -a ref.fa reads.fq | python -m svision_amd.sort - -o sorted.bam``: ``-`` is standard input (``<stdin>`` in messages),
and any path that os.stat says is no regular file -- a FIFO, /dev/fd/N, ``<(winnowmap -a ...)`` -- takes the same road, decided
before a byte is read.  The text is seen ONCE, and the two files are those of the same bytes read from a regular file:

  open      io.sam.StreamReader: the first bytes say what the stream holds (io.sam.stream_kind), the ``@`` lines are read up to the
            first line without ``@``; what was read beyond them stays in the reader's buffer
  key pass  the ONLY pass (:func:`_pipe_key_pass`): the reader's thread drains the pipe into two pinned buffers, chunks of ``range_bytes``
            cut by the rule of io.sam.chunk_places, while the device works on the chunk before; per chunk upload, svx_sam_lines,
            svx_sam_measure, the read-back, the host's lines -- all as for a file, with the stream's line numbers -- and AT ONCE
            svx_sam_encode into a SEGMENT of exactly the chunk's record bytes, the offsets the exclusive sum of the lengths behind the
            bytes kept so far.  Keys, fields, lengths, ``range_records`` and ``host_lens`` are kept as for a file
  the stream grows  by a segment a chunk: nothing is copied while the text arrives and nothing is allocated ahead, so what lies on the
            device is the record bytes seen so far -- a small pipe takes a small share of the card.  At the end of the input the
            segments are joined into the one resident stream (``Source.fill``; each goes when it is copied): then, and only then, both
            copies exist.  :func:`keeps_in_core` keeps a chunk while that join still fits ``memory_bytes``; so (a) the source's record
            buffers never exceed the budget, (b) never twice the record bytes seen plus one chunk's records -- and a pipe stays in core
            up to HALF the budget, where a file does up to all of it.  ``stats["stream_bytes"]``: the largest total, the join's
  the spool beyond it, the source switches to :class:`Spool` and does not fail: an unsorted BAM beside the output, ``out_path +
            ".spool.<pid>.bam"``, under the stream's header, written through :class:`BgzfWriter` with :class:`DeviceEncode` in the fixed
            code -- the records kept so far first, then every later chunk's as they are encoded, in arrival order (a chunk's buffer is
            in transit, like a span pass's chunk-local one, and not kept).  At the end of the input the pass's own results are dropped
            and the input BECOMES that file: the BAM road above, key pass, spans, ``again``.  One extra write and two reads of
            BAM-sized data, paid only by a pipe that does not fit
  among several inputs  a pipe is spooled from its first byte (``room`` is decided behind all key passes, and a pipe cannot be asked
            again), against the merged names and under the merged header, and is that file from ``_open_all`` on; its place in the
            list decides ties; without @SQ lines it is usable beside parts that have them.  ``-`` may appear once; further pipes of a run (FIFOs) spool to
            ``.spool.<pid>.<number>.bam`` and ``stats["pipes"]`` lists them all
  a BAM on a pipe  (``samtools view -b``, ``dorado aligner``, ``pbmm2``): BGZF or gzip magic whose inflated head is ``BAM\\1``.  By
            default the bytes are copied as they are into the spool file and the BAM road sorts that file -- one write and one read
            of compressed BAM more, room for it beside the output, and nothing runs on the device until the aligner has ended
  a BAM on a pipe, streamed  ``pipe_bam="stream"`` (``--pipe-bam stream``, ``SVX_PIPE_BAM=stream``; off by default: measured, it wins in
            core and loses once it spools, profiles/pipe_bam.txt and DESIGN section 9) takes a LONE such pipe in one pass (``BAM_PIPE_SOURCE``, :func:`_bam_pipe_key_pass`): the header
            through zlib from the stream (io.sam.StreamReader.bam_header), the BGZF members in chunks of ``range_bytes`` compressed
            bytes (textin.member_chunks: the reader's thread, pinned buffers), and per range the BAM key pass over index.stream_ranges,
            which carries a cut record's compressed blocks into the next range where a file's pass seeks back.  A range's records
            ``d_raw[first:exit_off]`` are a segment of exactly their size; :func:`keeps_in_core`, the spool beyond the budget (the
            kept records first, then every range's), the join and the statistics are the text pipe's.  In core no spool file exists
            at any moment.  Among several inputs a BAM pipe keeps the copy as it is under either setting: it would be spooled from its
            first byte anyway, and the copy is the cheapest form of that
  refused   other gzip data (compressed SAM: ``pigz -dc x.sam.gz | ... -`` is the road), no byte at all (``<stdin>: no input``)
On any failure the read end is closed BEFORE the error is raised -- standard input is pointed at the null device --, so that the
pipe's writer ends with EPIPE / SIGPIPE and does not block on a full pipe; no output, no temporary and no spool is left.  An early
end of the writer is no error by itself: what arrived is the input, and a cut last line fails by the parser's rules with its number.
``stats["pipe"]``: mode ("in_core", "spooled", "bam_spooled"), holds ("sam", "bam": what the pipe held), grows (segments + the join),
spool_bytes, text_bytes (the bytes read: of a BAM its compressed bytes, ``compressed_bytes`` too), and the seconds the reader's
thread waited for the pipe and for a free buffer.

Several inputs.  ``sort_bam([a.bam, b.sam, c.bam], out)`` -- ``python -m svision_amd.sort a.bam b.sam c.bam -o out.bam`` -- writes ONE sorted
BAM of all their records, what ``samtools merge`` in front of the sort would have given: one BAM per SMRT cell, one SAM per FASTQ batch.
The two files are, byte for byte, those of ONE unsorted BAM that holds the merged header and the inputs' records one input after the
other, every reference index in the merged numbering; ties of (reference, position) therefore come out in list order, then file order:
the stability of the one svx_record_sort over the inputs' keys end to end.

  open      every input as above; :func:`merge_headers` (host, its rules stand there) gives the output's text, its dictionary -- the
            union of the inputs' by name, in order of first appearance -- and per input the table old refID -> merged refID
  key pass  input by input in list order, each with its own header, first record and ranges: a BAM is walked against ITS OWN
            dictionary (svx_bam_find_starts validates against it).  Where its table is not the identity, svx_record_retid -- a lane a
            record -- rewrites refID and next_refID of the range's records where they lie, and the sort's key with them, before the
            slice is kept; the host's tid goes through the table in NumPy.  Identical dictionaries, or one that opens the merged
            one: no launch.  A reference index outside the file's dictionary: SortWriteError.  SAM text is measured and encoded
            against the MERGED names, so it needs no table, and a part without any header is usable beside one that has it
  join      ranges, keys and offsets of all inputs end to end: ``ranges`` and ``range_records`` of the statistics run over all of them
  spans     a span's ranges are read again input by input (``Source.again``), a BAM's records translated again before the scatter
  room      all inputs BAM: the sum of their ISIZE-derived rooms is known before the passes, the stream is allocated once, as for one
            file.  With SAM text among them the records' bytes are known only behind the key passes; they keep no byte, and a run
            that fits then fills the stream input by input -- the text encoded as for one SAM file, a BAM's ranges READ A SECOND TIME
            (``Source.fill``: the path of the spans without the scatter, one copy a range).  That second read is the price of a
            mixed run (profiles/sort_merge.txt); an all-BAM run does not pay it
A failure names the input it came from; "changed while it was sorted" names the input that changed.

A corrupt block, a CRC mismatch, a malformed or cut chain, a device allocation or a write that fails raises SortWriteError (a
ValueError); no file and no temporary is left behind.

:func:`sort_bam` is the list of its steps, each a function of this module over named values: ``_open_all`` (per input ``_open``: header,
first record and ``room`` from one pass over the file's members: index.bgzf_members, index.header_place; it also chooses the
:class:`Source`, BAM, SAM text or a pipe (``_open_pipe``): the key pass, the reading-again of a span's ranges and the filling of a stream whose size was not
known; several inputs: :func:`merge_headers`) -> ``_key_passes`` (per input its source's key pass, then ``_join``) -> ``_order`` -> the pieces,
``_pieces_in_core`` or ``_pieces_spanned``: generators of (device buffer, first byte, bytes), a chunk each -> :class:`BgzfWriter`,
which owns the temporary file and the ledger of members and is handed its encoder (:class:`DeviceEncode`; zlib in the CPU tests) ->
``_bai`` -> :func:`commit_pair`.  Which records a chunk or a span takes is one rule, :func:`records_touching`; the 0xFF00 cut one
function, :func:`block_cuts`.  How an input is opened and classified, a pipe's reader owned and closed, and a chunk of text read into
pinned memory and uploaded is svision_amd/textin.py's, shared with ingest_sort.load_sample; ``is_stream`` and ``input_paths`` live there.
"""
import collections
import os
import struct
import sys
import zlib

import numpy as np

from . import _lib, index, textin
from .textin import DEFAULT_SAM_CHUNK_BYTES, SAM_READ_THREADS, input_paths, is_stream    # noqa: F401  (their names here are in use)

BLOCK = 0xFF00                                                  # htslib's block size: inflated bytes a BGZF block of the output
DEFAULT_CHUNK_BYTES = 1024 * BLOCK
TABLES = ("fixed", "dynamic")                                   # the encoder: svx_bgzf_deflate / svx_bgzf_deflate_dyn
STAGES = ("read", "upload", "inflate", "crc", "find_starts", "walk", "scan", "read_back", "keep", "join", "sort", "gather", "scatter", "deflate",
          "pack", "download", "write", "index", "lines", "measure", "encode", "host_lines", "retid", "spool")


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


MergedHeader = collections.namedtuple("MergedHeader", "text references lengths maps")


def _line_fields(line):
    """A header line's TAG:VALUE fields -> {tag: value} (the first of a tag counts)."""
    out = {}
    for f in line.split("\t")[1:]:
        if len(f) > 2 and f[2] == ":":
            out.setdefault(f[:2], f[3:])
    return out


def _with_fields(line, new):
    """The line with the value of every field in ``new`` {tag: value} replaced, everything else as it is."""
    return "\t".join(f[:3] + new[f[:2]] if i and len(f) > 2 and f[2] == ":" and f[:2] in new else f for i, f in enumerate(line.split("\t")))


def merge_headers(parts):
    """The headers of several inputs -> MergedHeader(the merged text, through :func:`sorted_header_text`; the merged references and
    lengths; per input an int32 table ``map[old refID] -> merged refID``).  ``parts``: per input (its name for messages, the header
    text, its references, their lengths) -- the dictionary a BAM carries in binary, a SAM in its @SQ lines; a headerless SAM part has
    neither.  One input: its text through sorted_header_text and nothing else.  The rules:

      @HD   the first input's (sorted_header_text: SO:coordinate; none: one is prepended); a later input's is dropped
      @SQ   the union by SN in order of first appearance, the inputs taken in list order; the first occurrence's whole line is kept
            (a reference a BAM's text has no line for gets ``@SQ SN LN``); the same SN with another LN: SortWriteError
      @RG   the union by ID, an identical line once; the same ID on another line: SortWriteError (the records' RG:Z tags would have
            to be rewritten)
      @PG   the union by ID, an identical line once; the same ID on another line: the later input's line is renamed ID-<1-based input
            number>, and the PP fields of that input's other @PG lines follow.  The records' PG:Z tags are NOT rewritten
      other lines (@CO, ...): in input order, a line that is already there once
    A later input's new line goes behind the last line of its type so far (no such line: to the end), so the types stay together."""
    parts = [(name, text, list(refs), [int(v) for v in lens]) for name, text, refs, lens in parts]
    if len(parts) == 1:
        _name, text, refs, lens = parts[0]
        return MergedHeader(sorted_header_text(text), refs, lens, [np.arange(len(refs), dtype=np.int32)])
    out, seen, sq_seen = [], set(), set()                       # the merged lines, the lines that are there, the SN that have a line
    tid_of, owner, references, lengths, maps = {}, {}, [], [], []
    rg, pg = {}, {}                                             # ID -> (line, input's name)

    def add(line):
        at = next((i + 1 for i in range(len(out) - 1, -1, -1) if out[i][:3] == line[:3]), len(out))
        out.insert(at, line)
        seen.add(line)

    for k, (name, text, refs, lens) in enumerate(parts, 1):
        lines = [l for l in text.split("\n") if l.strip("\0")]
        # ---- the dictionary: the union by name, and this input's table
        table = np.empty(len(refs), np.int32)
        for i, (ref, n) in enumerate(zip(refs, lens)):
            if ref not in tid_of:
                tid_of[ref], owner[ref] = len(references), name
                references.append(ref)
                lengths.append(n)
            elif lengths[tid_of[ref]] != n:
                raise SortWriteError("%s and %s name the reference %s with different lengths: %d and %d -- they were not aligned to the "
                                     "same reference" % (owner[ref], name, ref, lengths[tid_of[ref]], n))
            table[i] = tid_of[ref]
        maps.append(table)
        # ---- @PG: which IDs of this input take the suffix (a rename changes the PP of other lines, which may rename those too)
        renamed = {}
        while k > 1:
            before = len(renamed)
            for l in lines:
                f = _line_fields(l) if l.startswith("@PG\t") else {}
                new = _with_fields(l, {"PP": renamed[f["PP"]]}) if f.get("PP") in renamed else l
                if f.get("ID") in pg and pg[f["ID"]][0] != new:
                    renamed[f["ID"]] = "%s-%d" % (f["ID"], k)
            if len(renamed) == before:
                break
        # ---- the lines: the first input's as they are, a later input's where they are new -- its new references first, in the
        # dictionary's order, then the rest in the text's
        sq_line = {}
        for l in lines:
            if l.startswith("@SQ\t"):
                sq_line.setdefault(_line_fields(l).get("SN"), l)

        def add_sq():
            for ref in refs:
                if ref not in sq_seen:
                    add(sq_line.get(ref) or "@SQ\tSN:%s\tLN:%d" % (ref, lengths[tid_of[ref]]))
                    sq_seen.add(ref)
        if k > 1:
            add_sq()
        for i, l in enumerate(lines):
            kind, f = l[:3], _line_fields(l)
            if kind == "@HD":
                if k == 1 and i == 0:
                    out.append(l)
                continue
            if kind == "@SQ":
                if k > 1:
                    continue
                sq_seen.add(f.get("SN"))
            if kind == "@RG" and "ID" in f:
                if k > 1 and f["ID"] in rg and rg[f["ID"]][0] != l:
                    raise SortWriteError("%s and %s both have a read group %s, on different @RG lines -- one of them would need its records' "
                                         "RG:Z tags rewritten, which this tool does not do: give the read groups distinct IDs"
                                         % (rg[f["ID"]][1], name, f["ID"]))
                rg.setdefault(f["ID"], (l, name))
            if kind == "@PG" and "ID" in f:
                change = {t: renamed[f[t]] for t in ("ID", "PP") if f.get(t) in renamed}
                l = _with_fields(l, change) if change else l
                pg.setdefault(renamed.get(f["ID"], f["ID"]), (l, name))
            if k == 1:
                out.append(l)
                seen.add(l)
            elif l not in seen:
                add(l)
        add_sq()                                                # (the first input's dictionary entries that its text has no line for)
    if not references:
        raise SortWriteError("%s: no input has an @SQ line: a BAM needs its reference dictionary" % parts[0][0])
    return MergedHeader(sorted_header_text("\n".join(out) + "\n"), references, lengths, maps)


def inflated_size(path):
    """The sum of the members' ISIZE fields: the file's inflated bytes, from its headers and footers alone."""
    try:
        return sum(isize for _at, _bsize, _xlen, isize in index.bgzf_members(path))
    except index.IndexBuildError as exc:
        raise SortWriteError(str(exc)) from None


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


def records_touching(off_out, lo, hi):
    """The records that touch the stream bytes [lo, hi), ``off_out`` [n + 1] being the records' offsets in the stream -> (r_lo, r_hi,
    base): the records [r_lo, r_hi) -- records of no byte between two others included, those at an edge left out: they have nothing
    to place -- and ``base = off_out[r_lo]``, the stream offset of the first one's first byte.  Scalars or arrays of lo and hi: the one
    rule of the chunks of a run in one piece and of the spans."""
    r_lo = np.searchsorted(off_out, lo, "right") - 1
    r_hi = np.searchsorted(off_out, hi, "left")
    return r_lo, r_hi, off_out[r_lo]


def plan_spans(off_out, memory_bytes):
    """The output's record stream [0, total), ``off_out`` [n + 1] being its records' offsets, cut into spans of
    ``max(memory_bytes // BLOCK, 1) * BLOCK`` bytes -- whole blocks, so the 0xFF00 cuts fall where they fall in one piece -> a list of
    Span(lo, hi, r_lo, r_hi, base, size): the stream bytes [lo, hi); the records [r_lo, r_hi) that touch them, by the rule of the
    chunks (:func:`records_touching`);
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
    r_lo, r_hi, base = records_touching(off_out, lo, hi)
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


# ---- a pipe's records: what is kept on the device, and the spool file beyond the budget (host) ----
STREAM_SLACK = 4                                                # readable bytes behind a record buffer: the gather's and the encoder's aligned loads


def keeps_in_core(kept, chunk, budget):
    """The growth rule of a pipe's record stream: ``kept`` record bytes lie on the device, a segment a chunk, and the next chunk brings
    ``chunk`` more -> whether it is kept too.  It is while the JOIN at the end of the input still fits the budget: the one buffer of
    kept + chunk + STREAM_SLACK bytes beside the segments it is copied from.  So (a) the segments, and the join's two copies, never
    exceed ``budget``; (b) every segment is exactly its chunk's records, so what is allocated is the record bytes seen so far until the
    join and twice that + STREAM_SLACK in it -- never beyond twice the bytes seen plus one chunk's records.  False: the spool."""
    return 2 * (int(kept) + int(chunk)) + STREAM_SLACK <= int(budget)


class StreamLedger:
    """The bytes of a source's record buffers on the device: ``now``, the largest total ``peak``, and how many times they grew."""

    def __init__(self):
        self.now = self.peak = self.grows = 0

    def add(self, n_bytes, grow=True):
        self.now += int(n_bytes)
        self.peak = max(self.peak, self.now)
        self.grows += bool(grow)

    def drop(self, n_bytes):
        self.now -= int(n_bytes)


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


# ---- the device steps ----
_Dev = collections.namedtuple("_Dev", "torch lib kernels dev clock")


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


# ``remap``: None, or the int32 table of :func:`merge_headers` that takes the input's reference indices into the merged dictionary
# (a BAM input of several whose table is not the identity: svx_record_retid).
# ``pipe``: None, or the :class:`_Pipe` the input came through -- still to be read (PIPE_SOURCE) or already in its spool file.
# ``text``: None, or the textin.TextInput whose chunks a SAM_SOURCE or PIPE_SOURCE reads.
Opened = collections.namedtuple("Opened", "path head first header room source remap pipe text", defaults=(None, None, None, None))
# The input's kind, chosen at open: ``key_pass(dv, opened, range_bytes, kp, d_stream)``: the input's ranges -> ``kp`` (the input's own
# KeyPass) filled, the records' bytes kept in ``d_stream`` from byte ``kp.base`` on where it is given; ``again(dv, opened, kp, need) ->
# per range of ``need`` (k, records completed, device bytes, the records' offsets in them [n + 1])``, the ranges of the key pass read
# once more for a span; ``fill(dv, opened, kp)``: the input's records written into ``kp.d_stream`` behind the key passes (a run in one
# piece whose ``room`` was not known before them).
Source = collections.namedtuple("Source", "name key_pass again fill")
# Every input opened, and the one file they make: ``merged`` is an Opened whose head (references, lengths), header bytes and room are
# the output's -- of one input: that input's own --, ``label`` names the inputs in a message.
Inputs = collections.namedtuple("Inputs", "opened merged label")
MergedHead = collections.namedtuple("MergedHead", "references lengths")


# What the steps of one run share besides the device: where the output goes (a spool lies beside it), the output's chunk, the budget
# for the records' bytes, ``pipes``: every :class:`_Pipe` the run opened, for sort_bam to close and to clean up behind, and the clock.
# ``stream_bam``: a lone BAM on a pipe is taken in one pass (``pipe_bam="stream"``), not copied into a file first.
_Run = collections.namedtuple("_Run", "out_path chunk_blocks budget range_bytes pipes clock stream_bam", defaults=(False,))


def _open_all(paths, dv=None, run=None):
    """open, every input: -> Inputs.  One input: as it is opened.  Several: the headers merged (:func:`merge_headers`) -- a SAM part
    takes the merged dictionary for its own, so its records are encoded in the merged numbering and a part without header is
    usable; a BAM part whose table is not the identity carries it as ``remap`` --, ``room`` the sum where every part's is known."""
    from .io import sam
    if paths.count("-") > 1:
        raise SortWriteError("%s is named twice: standard input is one stream" % sam.STREAM_NAME)
    if len(paths) == 1:
        opened = _open(paths[0], run=run)
        return Inputs([opened], opened, opened.path if opened.pipe is None else opened.pipe.name)
    opened = [_open(p, alone=False, run=run) for p in paths]
    merged = merge_headers([(o.path, o.head.text if o.source in (SAM_SOURCE, PIPE_SOURCE) else o.head.header_text, o.head.references, o.head.lengths) for o in opened])
    header = sam.bam_header_bytes(sam.SamHead(merged.references, merged.lengths, merged.text, "coordinate"))
    for i, o in enumerate(opened):
        if o.source in (SAM_SOURCE, PIPE_SOURCE):               # text: measured and encoded against the merged names
            opened[i] = o = o._replace(head=sam.SamHead(merged.references, merged.lengths, o.head.text, o.head.sort_order))
            if o.source is PIPE_SOURCE:                         # a pipe among several: spooled from its first byte, under the merged header
                opened[i] = _pipe_spooled(dv, o, header)
        elif not np.array_equal(merged.maps[i], np.arange(len(merged.maps[i]))):       # (a dictionary that opens the merged one: nothing to rewrite)
            opened[i] = o._replace(remap=merged.maps[i])
    rooms = [o.room for o in opened]
    label = "%s (+ %d more)" % (paths[0], len(paths) - 1)
    return Inputs(opened, Opened(label, MergedHead(merged.references, merged.lengths), None, header,
                                 None if None in rooms else sum(rooms), None), label)


_COMPRESSED_SAM = ("%s: gzip- or BGZF-compressed data that is no BAM -- compressed SAM is not taken: decompress it, or convert it with "
                   "`samtools view -b`; through a pipe it is: `pigz -dc x.sam.gz | python -m svision_amd.sort - -o sorted.bam`")


def _open(bam_path, alone=True, run=None):
    """open: -> Opened(the path, read_bam_header's table, first_record's (file offset, entry, references), the header's bytes as the
    output takes them, ``room``: the records' inflated bytes by the members' ISIZE fields) -- one pass over the file's members.  SAM
    text (a first byte ``@``, or a first line of 11 tab-separated fields): :func:`_open_sam`; read once: :func:`_open_pipe`."""
    from .io import sam
    from .io.bam import read_bam_header
    if run is None and is_stream(bam_path):
        raise SortWriteError("%s: not a regular file" % bam_path)
    try:
        inp = textin.open_input(bam_path)
    except (sam.SamError, OSError) as exc:
        raise SortWriteError("%s: %s" % (textin.name_of(bam_path), exc)) from None
    if inp.kind != "bam":
        return _open_sam(inp, alone) if inp.kind == "sam" else _open_pipe(inp, alone, run)
    if inp.peek_kind == sam.STREAM_GZIP:
        raise SortWriteError(_COMPRESSED_SAM % bam_path)
    try:
        head = read_bam_header(bam_path)
        members = index.bgzf_members(bam_path)
        place = index.header_place(bam_path, members)           # (takes the members the header lies in; the rest follow below)
        header = sorted_header_bytes(place.head)
        room = place.isize + sum(isize for _at, _bsize, _xlen, isize in members) - len(place.head)
    except (ValueError, TypeError, OSError, zlib.error, struct.error) as exc:
        raise SortWriteError("%s: %s" % (bam_path, exc)) from None
    if room < 0:
        raise SortWriteError("%s: its BGZF blocks hold fewer bytes than its header" % bam_path)
    return Opened(bam_path, head, tuple(place[:3]), header, room, BAM_SOURCE)


def _open_sam(inp, alone=True, pipe=None):
    """open, SAM text -- a file's, or (``pipe``) what waits in a pipe behind its ``@`` lines: -> Opened(the input's name, the header's
    references and lengths (io.sam.SamHead), (the bytes, the lines) in front of the first alignment line, the output's header bytes,
    ``room`` None: the records' bytes are known behind the key pass).  One of several inputs (``alone`` unset) may have no @SQ line:
    the other parts' dictionary serves it."""
    from .io import sam
    bare = not alone and inp.headerless
    try:
        head = sam.SamHead([], [], inp.text.decode("latin-1"), None) if bare else sam.parse_header(inp.text)
    except sam.SamError as exc:
        raise SortWriteError("%s: %s" % (inp.name, exc)) from None
    return Opened(inp.name, head, inp.first, None if bare else sorted_header_bytes(sam.bam_header_bytes(head)), None,
                  SAM_SOURCE if pipe is None else PIPE_SOURCE, None, pipe, inp)


class KeyPass:
    """What the pass over the file leaves, filled by :func:`_key_pass` as it goes (``seen`` is right in a failure's message too):
    ``range_records`` and ``places`` per range; ``seen``: the inflated record bytes so far; behind the join the ``n`` records' host
    fields ``tid pos flag span``, the device keys ``d_tid d_pos`` (until the sort has taken them), the records' offsets in the joined
    stream ``off_in`` / ``d_off_in`` [n + 1], and ``d_stream``: the resident record stream, None in a spanned run.  SAM text besides:
    ``host_lens`` per chunk the lines' lengths as svx_sam_encode takes them (negative: the host's line), ``host_records`` {record
    number: the bytes io.sam encoded}, ``tid_of`` / ``sam_table``: the host's and the device's reference names, ``reader``: the
    textin.ChunkReader of the text, with the pinned memory a chunk is read into."""

    def __init__(self, base=0):
        self.range_records, self.places, self.seen, self.n = [], [], 0, 0
        self.host_lens, self.host_records, self.tid_of, self.sam_table, self.reader = [], {}, None, None, None
        self.tid = self.pos = self.flag = self.span = self.d_tid = self.d_pos = self.off_in = self.d_off_in = self.d_stream = None
        # Several inputs: the run's KeyPass holds the joined arrays and, in ``parts``, per input (its Opened, its own KeyPass, the
        # number of its first range and of its first record in the run); an input's own KeyPass has its ranges, what the join takes of
        # them (``host``, ``d_keys``, ``lens``: per range the host fields, the device keys, the records' lengths), ``base``: the stream
        # offset of its first record, and behind the join its slices of ``off_in`` / ``d_off_in`` -- offsets in the one stream.
        # ``reading``: the input that is being read, for a failure's message.
        self.parts, self.host, self.d_keys, self.lens, self.base, self.reading, self.d_map = [], [], [], [], base, None, None


def _retid(dv, opened, kp, d_bytes, d_off, d_tid_key):
    """The records at ``d_off`` in ``d_bytes`` of an input whose reference indices are not the merged dictionary's: refID and next_refID
    -- and the sort's key -- through the input's table (svx_record_retid)."""
    torch = dv.torch
    if kp.d_map is None:
        kp.d_map = torch.from_numpy(np.ascontiguousarray(opened.remap, np.int32)).to(dv.dev)
    d_status = torch.zeros(1, dtype=torch.int32, device=dv.dev)
    dv.kernels.record_retid(d_bytes, d_off, kp.d_map, d_tid_key, d_status)
    bad = int(d_status.item())
    dv.clock.lap("retid")
    if bad:
        raise SortWriteError("%s: a record's reference index is outside its file's dictionary (%d references)" % (opened.path, len(opened.remap)))


def _key_pass(dv, opened, range_bytes, kp, d_stream):
    """key pass of a BAM: every range of the file (index.record_ranges) -> ``kp`` filled.  ``d_stream``: the record stream, allocated
    once by the ISIZE sum -- every range's slice goes straight to its place in it, from byte ``kp.base`` on --, or None: no byte is
    kept.  An input with a ``remap``: the range's records and keys are translated where they lie (:func:`_retid`), the host's tid too."""
    torch, dev, clock, room = dv.torch, dv.dev, dv.clock, opened.room
    for rng in index.record_ranges(opened.path, opened.head, dev, clock, range_bytes, first=opened.first):
        kp.range_records.append(int(rng.n_rec))
        kp.places.append(rng.place)
        if rng.n_rec:
            tid, pos, flag, span, rec_off = index._index_fields(dv.lib, torch, dv.kernels, dev, rng, clock)
            first, last = int(rec_off[0]), int(rng.exit_off)
            if kp.seen + last - first > room:
                raise SortWriteError("%s: more record bytes than its BGZF blocks' ISIZE fields add up to (%d)" % (opened.path, room))
            if opened.remap is not None:
                _retid(dv, opened, kp, rng.d_raw, rng.d_rec_off, rng.d_tid)
                tid = np.where(tid >= 0, opened.remap[np.maximum(tid, 0)], tid).astype(np.int32)
            kp.host.append((tid, pos, flag, span))
            kp.lens.append(np.diff(np.append(rec_off, np.uint64(last)).astype(np.int64)))
            kp.d_keys.append((rng.d_tid, rng.d_pos))
            if d_stream is not None:
                at = kp.base + kp.seen
                d_stream[at:at + last - first].copy_(rng.d_raw[first:last])      # the records that complete in the range: contiguous there
            kp.seen += last - first
        rng.d_raw = rng.d_starts = rng.d_base = rng.d_cigar = rng.d_cig_off = rng.d_names = rng.d_name_off = rng.d_rec_off = None
        del rng
        clock.lap("keep")


def _key_passes(dv, ins, budget, range_bytes):
    """key pass, every input in list order -> (the merged Opened with its ``room`` known, the run's KeyPass joined, ``spanned``).  Where
    every input's ``room`` is known before (BAMs: the ISIZE sums), the records are kept as the passes go wherever they fit the budget.
    With SAM text among the inputs ``room`` is exact only behind the passes: they keep no byte, and a run that fits then fills the
    stream input by input (``Source.fill``: the text encoded, a BAM's ranges read a second time, one copy a range)."""
    torch, dev = dv.torch, dv.dev
    kp, merged = KeyPass(), ins.merged
    known = merged.room is not None
    spanned = known and merged.room > budget                    # the records do not fit: no byte is kept in the pass, the output is filled in spans
    if known and not spanned:
        kp.d_stream = torch.empty(merged.room + 4, dtype=torch.uint8, device=dev)      # (4 readable bytes behind it: the gather's aligned loads)
    ranges = records = 0
    for opened in ins.opened:
        part = KeyPass(kp.seen)
        kp.parts.append((opened, part, ranges, records))
        kp.reading = opened.path
        opened.source.key_pass(dv, opened, range_bytes, part, kp.d_stream)
        if (opened.source is PIPE_SOURCE or opened.source is BAM_PIPE_SOURCE) and opened.pipe.mode == "spooled":
            # the pipe did not fit: what its pass kept is dropped, the input becomes its spool file and takes the road of a BAM
            again = _open(opened.pipe.spool_file)._replace(pipe=opened.pipe)
            del part, kp
            return _key_passes(dv, Inputs([again], again, ins.label), budget, None)
        kp.seen += part.seen
        ranges, records = ranges + len(part.range_records), records + sum(part.range_records)
    kp.reading = None
    _join(dv, merged, kp)
    if not known:
        merged = merged._replace(room=int(kp.off_in[-1]))
        spanned = merged.room > budget
        if not spanned:
            kp.d_stream = torch.empty(merged.room + 4, dtype=torch.uint8, device=dev)
            kp.d_stream[merged.room:] = 0
            for opened, part, _ranges, _records in kp.parts:
                kp.reading, part.d_stream = opened.path, kp.d_stream
                opened.source.fill(dv, opened, part)
            kp.reading = None
    return merged, kp, spanned


def _join(dv, opened, kp):
    """join: what the inputs' ranges left -- per range the host fields, the device keys and the records' lengths -> ``kp``'s arrays of
    the one record stream, and every input's slices of the offsets."""
    torch, dev, clock = dv.torch, dv.dev, dv.clock
    host, d_keys, lens = ([v for _o, part, _r, _n in kp.parts for v in getattr(part, name)] for name in ("host", "d_keys", "lens"))
    kp.range_records = [v for _o, part, _r, _n in kp.parts for v in part.range_records]
    kp.places = [v for _o, part, _r, _n in kp.parts for v in part.places]
    n = kp.n = int(sum(l.size for l in lens))
    if n > 0xFFFFFFFF:
        raise SortWriteError("%s: %d records -- svx_record_sort takes up to 2^32 - 1" % (opened.path, n))
    # ---- join: CSR offsets and the keys of the one record stream
    if kp.d_stream is not None:
        kp.d_stream[kp.seen:] = 0
    kp.off_in = np.zeros(n + 1, np.int64)
    if n:
        kp.off_in[1:] = np.cumsum(np.concatenate(lens))
    kp.d_off_in = torch.from_numpy(kp.off_in).to(dev)
    if n:
        kp.d_tid, kp.d_pos = torch.cat([k[0] for k in d_keys]), torch.cat([k[1] for k in d_keys])
        kp.tid, kp.pos, kp.flag, kp.span = (np.concatenate([h[i] for h in host]) for i in range(4))
    else:
        kp.d_tid = kp.d_pos = torch.empty(0, dtype=torch.int32, device=dev)
        kp.tid = kp.pos = kp.span = np.empty(0, np.int32)
        kp.flag = np.empty(0, np.uint16)
    del d_keys, host, lens
    for _o, part, _r, first in kp.parts:
        part.n = int(sum(part.range_records))
        part.off_in, part.d_off_in = kp.off_in[first:first + part.n + 1], kp.d_off_in[first:first + part.n + 1]
        part.host, part.d_keys, part.lens = [], [], []
    clock.lap("join")
    return kp


Ordered = collections.namedtuple("Ordered", "order off_out d_order d_off_out pos_bits rank d_rank plan spans stream_bytes")


def _order(dv, opened, kp, spanned, budget):
    """order: ONE svx_record_sort over the keys (they go with it) -> Ordered(the records in output order, ``order`` / ``d_order`` [n];
    their offsets in the output stream, ``off_out`` / ``d_off_out`` [n + 1]; ``pos_bits``; for a spanned run every input record's
    ``rank`` / ``d_rank`` and the ``plan`` of :func:`plan_spans`, else None; the number of ``spans``, 1 in one piece; ``stream_bytes``:
    the largest record buffer of the run)."""
    from . import ingest_sort
    torch, kernels, dev, n = dv.torch, dv.kernels, dv.dev, kp.n
    pos_bits = ingest_sort.pos_bits_for(opened.head.lengths, int(kp.pos.max()) if n else -1)
    if n:
        d_order = kernels.record_sort(kp.d_tid, kp.d_pos, len(opened.head.references), pos_bits)
        d_off_out = kernels.record_gather_offsets(kp.d_off_in, d_order)
    else:                                                       # a header and no record: header blocks + the end-of-file marker
        d_order, d_off_out = torch.empty(0, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    order = d_order.cpu().numpy().view(np.uint32).astype(np.int64)
    off_out = d_off_out.cpu().numpy()
    kp.d_tid = kp.d_pos = None
    dv.clock.lap("sort")
    if not spanned:
        return Ordered(order, off_out, d_order, d_off_out, pos_bits, None, None, None, 1, int(kp.d_stream.numel()))
    d_rank = kernels.record_invert(d_order)
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n, dtype=np.int64)
    plan = plan_spans(off_out, budget)
    dv.clock.lap("sort")
    return Ordered(order, off_out, d_order, d_off_out, pos_bits, rank, d_rank, plan, len(plan), max((sp.size for sp in plan), default=0))


def _pieces_in_core(dv, opened, kp, od, chunk_blocks, counts):
    """pieces of a run in one piece: per chunk the records that touch it gathered from the resident stream -> (device buffer, the
    chunk's first byte in it, its bytes).  The buffer goes before the next one is allocated: the caller drops its piece first."""
    torch, lib, dev = dv.torch, dv.lib, dv.dev
    st = dv.kernels._stream_ptr(dev)
    for lo, hi in chunk_cuts(0, int(od.off_out[-1]), chunk_blocks * BLOCK):
        r_lo, r_hi, base = (int(v) for v in records_touching(od.off_out, lo, hi))
        d_rebased = od.d_off_out[r_lo:r_hi + 1] - base
        d_rows = od.d_order[r_lo:r_hi].contiguous()
        d_chunk = torch.empty(int(od.off_out[r_hi]) - base + 4, dtype=torch.uint8, device=dev)
        _lib.check(lib.svx_record_gather_segments(kp.d_stream.data_ptr(), kp.d_off_in.data_ptr(), d_rows.data_ptr(), d_rebased.data_ptr(),
                                                  d_chunk.data_ptr(), r_hi - r_lo, 1, st), "svx_record_gather_segments")
        dv.clock.lap("gather")
        yield d_chunk, lo - base, hi - lo
        del d_chunk


def _pieces_spanned(dv, opened, kp, od, chunk_blocks, counts):
    """pieces of a run in spans: the record stream in pieces of the budget, each filled by a pass over the ranges that own its records
    (``counts["span_range_reads"]`` of them in all; the source reads them again: :func:`_bam_again`, :func:`_sam_again`) and then
    given chunk by chunk -> as :func:`_pieces_in_core`."""
    torch, lib, kernels, dev, clock = dv
    rec_base = _rec_base(kp)
    for sp in od.plan:
        d_span = torch.empty(sp.size, dtype=torch.uint8, device=dev)
        need = span_ranges(od.rank, kp.range_records, sp.r_lo, sp.r_hi)
        clock.lap("scatter")
        for part_of, part, first_range, _first_record in kp.parts:             # input by input: each reads its own ranges again
            mine = need[(need >= first_range) & (need < first_range + len(part.range_records))] - first_range
            d_status = torch.zeros(1, dtype=torch.int32, device=dev)
            kp.reading = part_of.path
            for k_own, n_rec, d_raw, d_src_off in part_of.source.again(dv, part_of, part, mine) if mine.size else ():
                k = first_range + int(k_own)
                counts["span_range_reads"] += 1
                if n_rec != kp.range_records[k]:
                    raise SortWriteError("%s changed while it was sorted: %d records complete in the range at file offset %d, %d did in the "
                                         "first pass" % (part_of.path, n_rec, kp.places[k][0], kp.range_records[k]))
                kernels.record_scatter_segments(d_raw, d_src_off, od.d_rank[int(rec_base[k]):int(rec_base[k + 1])], sp.r_lo, sp.r_hi,
                                                od.d_off_out, sp.base, d_span, d_status)
                clock.lap("scatter")
                del d_raw, d_src_off
            if mine.size and int(d_status.item()):
                raise SortWriteError("%s changed while it was sorted: a record's length is not the one the first pass saw" % part_of.path)
        kp.reading = None
        for lo, hi in chunk_cuts(sp.lo, sp.hi, chunk_blocks * BLOCK):
            yield d_span, lo - sp.base, hi - lo
        del d_span


# ---- the sources: a BAM's ranges, a SAM's chunks of text ----
def _rec_base(kp):
    """The number of the first record of every range of the key pass, and behind the last [ranges + 1]."""
    return np.concatenate([[0], np.cumsum(np.asarray(kp.range_records, np.int64))])


def _bam_again(dv, opened, kp, need):
    """The ranges ``need`` of a BAM read again: read, inflate, CRC, find_starts, the walk's counts and offsets; nothing is extracted.
    An input with a ``remap``: the range's records translated where they lie before they are handed on (:func:`_retid`)."""
    for k, rng in zip(need, index.record_ranges(opened.path, opened.head, dv.dev, dv.clock, places=[kp.places[k] for k in need], extract=False,
                                                first=opened.first)):
        if rng.n_rec != kp.range_records[k]:
            yield k, rng.n_rec, None, None                      # (the caller refuses it; no offsets are taken of a range that changed)
            return
        d_src_off = index.walk_offsets(dv.lib, dv.torch, dv.kernels, dv.dev, rng, closed=True)
        dv.clock.lap("walk")
        if opened.remap is not None:
            _retid(dv, opened, kp, rng.d_raw, d_src_off[:rng.n_rec], None)
        yield k, rng.n_rec, rng.d_raw, d_src_off
        rng.d_raw = rng.d_starts = rng.d_base = None
        del rng, d_src_off


def _bam_fill(dv, opened, kp):
    """in one piece, a BAM beside SAM text (``room`` was not known before the key passes): the ranges that completed a record read a
    second time, each range's records -- contiguous in the range and in the stream -- one copy."""
    need = np.flatnonzero(np.asarray(kp.range_records, np.int64))
    rec_base = _rec_base(kp)
    for k, n_rec, d_raw, d_src_off in _bam_again(dv, opened, kp, need) if need.size else ():
        ends = [int(v) for v in d_src_off[[0, n_rec]].cpu()] if n_rec == kp.range_records[k] else None
        at, end = int(kp.off_in[rec_base[k]]), int(kp.off_in[rec_base[k + 1]])
        if ends is None or ends[1] - ends[0] != end - at:
            raise SortWriteError("%s changed while it was sorted: the range at file offset %d does not complete the records it did in the "
                                 "first pass" % (opened.path, kp.places[k][0]))
        kp.d_stream[at:end].copy_(d_raw[ends[0]:ends[1]])
        dv.clock.lap("keep")
        del d_raw, d_src_off


Measured = collections.namedtuple("Measured", "first length kernel_len tid pos flag span d_tid d_pos")


def _sam_measured(dv, opened, kp, chunk, d_text, d_line_off, n_lines):
    """A chunk's lines measured (svx_sam_measure) and read back -> Measured(the number of the chunk's first record, the records' lengths
    with the host's lines patched in, the lengths as svx_sam_encode takes them, tid, pos, flag, span on the host, the keys on the device).
    An error code raises with the line's number -- ``chunk.line_no`` lines lie in front of the chunk --; a line the kernels leave to the
    host is encoded by io.sam.encode_line and kept in ``kp.host_records`` by record number.  A pass's first call sets ``kp``'s names."""
    from .io import sam
    if kp.sam_table is None:
        kp.tid_of, kp.sam_table = sam.tid_table(opened.head.references), dv.kernels.sam_ref_table(opened.head.references, dv.dev)
    torch, kernels, dev, clock = dv.torch, dv.kernels, dv.dev, dv.clock
    d_len, d_tid, d_pos, d_flag, d_span = kernels.sam_measure(d_text, chunk.n, d_line_off, n_lines, kp.sam_table)
    clock.lap("measure")
    length, tid, pos, flag, span = (t.cpu().numpy() for t in (d_len, d_tid, d_pos, d_flag, d_span))
    line_off = d_line_off[:n_lines + 1].cpu().numpy()
    clock.lap("read_back")
    bad = np.flatnonzero(length < kernels.SAM_HOST)
    if bad.size:
        i = int(bad[0])
        raise SortWriteError("%s: %s" % (opened.path, textin.line_refusal(textin.line_bytes(chunk.data, line_off, i), kp.tid_of, chunk.line_no + i + 1,
                                                                      "svx_sam_measure", int(length[i]))))
    kernel_len, first = length.copy(), sum(kp.range_records)
    left = np.flatnonzero(length == kernels.SAM_HOST)
    for i in left:
        line = textin.line_bytes(chunk.data, line_off, i)
        try:
            rec = sam.encode_line(line, kp.tid_of)
            tid[i], pos[i], flag[i], span[i] = sam.fields_of(line, kp.tid_of)
        except sam.SamError as exc:
            raise SortWriteError("%s: %s" % (opened.path, exc.at(chunk.line_no + int(i) + 1))) from None
        length[i] = len(rec)
        kp.host_records[first + int(i)] = rec
    if left.size:
        d_tid, d_pos = torch.from_numpy(tid).to(dev), torch.from_numpy(pos).to(dev)
    clock.lap("host_lines", False)
    return Measured(first, length.astype(np.int64), kernel_len, tid, pos, flag.astype(np.uint16), span, d_tid, d_pos)


def _keep_measured(kp, place, m, keys=True):
    """A measured chunk into the input's KeyPass; ``keys`` unset (its records go to a spool): without what the join takes of it."""
    kp.range_records.append(m.length.size)
    kp.places.append(place)
    kp.host_lens.append(m.kernel_len)
    if keys and m.length.size:
        kp.host.append((m.tid, m.pos, m.flag, m.span))
        kp.lens.append(m.length)
        kp.d_keys.append((m.d_tid, m.d_pos))
    kp.seen += int(m.length.sum())


def _place_host_records(torch, take, kernel_len, first, off, d_out):
    """A chunk's records that the host encoded (``kernel_len`` < 0), ``take(first + i)`` each, copied to ``off[i]`` in ``d_out`` -> how many."""
    left = np.flatnonzero(kernel_len < 0)
    for i in left:
        rec = take(first + int(i))
        d_out[int(off[i]):int(off[i]) + len(rec)].copy_(torch.frombuffer(bytearray(rec), dtype=torch.uint8))
    return left.size


def _sam_key_pass(dv, opened, range_bytes, kp, d_stream=None):
    """key pass of SAM text: one pass over the chunks (textin.ChunkReader.chunks: ``range_bytes`` of text, cut at line ends): svx_sam_lines,
    svx_sam_measure, the lengths and fields read back.  An error code raises with the file's line number; a line the kernels leave to the
    host (SVX_SAM_HOST) is encoded by io.sam at once -- its bytes kept in ``kp.host_records`` by record number, its length, key and
    fields patched in.  No byte is kept: ``room`` is exact behind the pass, and a run in one piece then reads the text once more
    (:func:`_sam_fill`)."""
    kp.reader = textin.ChunkReader(dv.torch, dv.lib, dv.clock)
    for chunk in kp.reader.chunks(opened.text, range_bytes):
        d_text, d_line_off, n_lines = textin.upload_lines(dv.torch, dv.kernels, dv.dev, dv.clock, chunk)
        _keep_measured(kp, chunk.place, _sam_measured(dv, opened, kp, chunk, d_text, d_line_off, n_lines))
        del d_text, d_line_off
        dv.clock.lap("keep")


def _sam_encode_chunk(dv, opened, kp, k, first, base, d_out, d_status):
    """Chunk k of the key pass read again and its records written: svx_sam_lines -> svx_sam_encode to ``d_out``, record r of the stream
    at byte off_in[r] - base; the host's encodings copied to their offsets.  ``first``: the number of the chunk's first record.
    -> the lines the chunk has now (another number than in the key pass: nothing is written)."""
    torch, kernels = dv.torch, dv.kernels
    try:
        chunk = kp.reader.at(opened.text, kp.places[k])
    except textin.ReadError as exc:
        raise SortWriteError("%s changed while it was sorted: %s" % (exc.path, exc.what)) from None
    d_text, d_line_off, n_lines = textin.upload_lines(torch, kernels, dv.dev, dv.clock, chunk)
    if n_lines != kp.range_records[k]:
        return n_lines
    d_len = torch.from_numpy(kp.host_lens[k]).to(dv.dev)
    kernels.sam_encode(d_text, chunk.n, d_line_off, n_lines, kp.sam_table, d_len, kp.d_off_in[first:first + n_lines], base, d_out, d_status)
    dv.clock.lap("encode")
    _place_host_records(torch, kp.host_records.__getitem__, kp.host_lens[k], first, kp.off_in[first:first + n_lines] - base, d_out)
    dv.clock.lap("host_lines")
    return n_lines


def _sam_fill(dv, opened, kp):
    """in one piece, SAM text: the second read of the text -- in the page cache for a file that fits the device --, every chunk encoded
    straight into the resident stream (``kp.d_stream``) at its records' offsets."""
    d_status = dv.torch.zeros(1, dtype=dv.torch.int32, device=dv.dev)
    for k, first in enumerate(_rec_base(kp)[:-1]):
        n_lines = _sam_encode_chunk(dv, opened, kp, k, int(first), 0, kp.d_stream, d_status)
        if n_lines != kp.range_records[k]:
            raise SortWriteError("%s changed while it was sorted: %d lines complete in the chunk at file offset %d, %d did in the first pass"
                                 % (opened.path, n_lines, kp.places[k][0], kp.range_records[k]))
    if int(d_status.item()):
        raise SortWriteError("%s changed while it was sorted: a line's record is not of the length the first pass saw" % opened.path)


def _sam_again(dv, opened, kp, need):
    """The chunks ``need`` of SAM text read again for a span: each encoded into a chunk-local buffer (+ the 4 readable bytes the
    scatter's aligned loads want) whose record offsets are the key pass's."""
    torch, dev = dv.torch, dv.dev
    rec_base = _rec_base(kp)
    for k in need:
        first, n_rec = int(rec_base[k]), int(kp.range_records[k])
        base = int(kp.off_in[first])
        d_local = torch.zeros(int(kp.off_in[first + n_rec]) - base + 4, dtype=torch.uint8, device=dev)
        d_status = torch.zeros(1, dtype=torch.int32, device=dev)
        d_src_off = kp.d_off_in[first:first + n_rec + 1] - base
        n_lines = _sam_encode_chunk(dv, opened, kp, k, first, base, d_local, d_status)
        if n_lines == n_rec and int(d_status.item()):
            raise SortWriteError("%s changed while it was sorted: a line's record is not of the length the first pass saw" % opened.path)
        yield k, n_lines, d_local, d_src_off
        del d_local, d_src_off


# ---- a pipe: SAM text that is seen once ----
class _Pipe:
    """An input that is read once -- standard input, a FIFO, /dev/fd/N -- as the sort keeps it: the textin.TextInput that owns its
    reader, its name in messages (``<stdin>`` for ``-``), ``mode`` ("in_core", "spooled", "bam_spooled"), the ledger of its record
    buffers on the device, its segments (a chunk's records each) while it is kept in core, its :class:`Spool` beyond the budget, and
    what the statistics report.  :meth:`discard` removes the spool; closing is the input's (textin.TextInput.close)."""

    def __init__(self, inp, run):
        self.input, self.name, self.run, self.number = inp, inp.name, run, len(run.pipes)
        self.mode, self.ledger, self.segments, self.spool, self.spool_file = "in_core", StreamLedger(), [], None, None
        self.spool_bytes = self.host_lines = 0
        self.holds, self.bam_header = "sam", None               # what the pipe held; a streamed BAM: the bytes in front of its first record

    def discard(self):
        self.segments = []
        if self.spool is not None:
            self.spool.discard()
        index.discard(self.spool_file)

    def stats(self):
        reader = self.input.reader
        return dict(mode=self.mode, holds=self.holds, grows=self.ledger.grows, spool_bytes=self.spool_bytes, text_bytes=reader.text_bytes,
                    reader_wait_pipe_s=round(reader.wait_pipe, 6), reader_wait_buffer_s=round(reader.wait_buffer, 6),
                    **(dict(compressed_bytes=reader.text_bytes) if self.holds == "bam" else {}))


def _open_pipe(inp, alone, run):
    """open, an input that is read once, by what its first bytes hold.  SAM text: :func:`_open_sam`'s Opened, its source PIPE_SOURCE,
    the text waiting in the pipe.  A BAM: copied as it is into the spool file, which is opened as any BAM -- or, alone and under
    ``run.stream_bam``, its header read from the stream and the rest left waiting for BAM_PIPE_SOURCE.  Anything else: refused."""
    from .io import sam
    pipe = _Pipe(inp, run)
    run.pipes.append(pipe)
    refusal = {sam.STREAM_EMPTY: "%s: no input", sam.STREAM_GZIP: _COMPRESSED_SAM, sam.STREAM_OTHER: "%s: neither SAM text nor a BAM"}
    if inp.peek_kind in refusal:
        raise SortWriteError(refusal[inp.peek_kind] % inp.name)
    if inp.peek_kind == sam.STREAM_SAM:
        return _open_sam(inp, alone, pipe)
    pipe.holds = "bam"
    if alone and run.stream_bam:
        try:
            got = inp.reader.bam_header()
            pipe.bam_header = got.head
            return Opened(inp.name, got.table, got.first, sorted_header_bytes(got.head), None, BAM_PIPE_SOURCE, None, pipe, inp)
        except (sam.BgzfStreamError, ValueError, struct.error) as exc:
            raise SortWriteError("%s: %s" % (inp.name, exc)) from None
    pipe.mode = "bam_spooled"
    try:
        pipe.spool_file, pipe.spool_bytes = spool_copy(inp.reader, run.out_path, run.clock, pipe.number)
    except OSError as exc:
        raise SortWriteError("%s: %s" % (inp.name, exc)) from None
    inp.close()
    return _open(pipe.spool_file, alone)._replace(pipe=pipe)


def _pipe_join(dv, pipe, d_out, at=0):
    """The segments of a pipe kept in core, end to end into ``d_out`` from byte ``at`` on; each goes when it is copied."""
    for k, d_seg in enumerate(pipe.segments):
        d_out[at:at + d_seg.numel()].copy_(d_seg)
        at += d_seg.numel()
        pipe.segments[k] = None
        pipe.ledger.drop(d_seg.numel())
        del d_seg
    pipe.segments = []
    dv.clock.lap("keep")
    return at


def _pipe_to_spool(dv, opened, kp, header):
    """The budget does not hold the next chunk (or the pipe is one of several inputs): the spool file is opened with ``header``, and
    the records kept so far go in first -- joined into one buffer, which the rule of :func:`keeps_in_core` has left room for."""
    torch, pipe = dv.torch, opened.pipe
    pipe.mode = "spooled"
    pipe.spool = Spool(pipe.run.out_path, header, DeviceEncode(dv, "fixed"), dv.clock,
                       lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(dv.dev), pipe.name, pipe.number)
    if pipe.segments:
        d_kept = torch.empty(kp.seen + STREAM_SLACK, dtype=torch.uint8, device=dv.dev)
        pipe.ledger.add(d_kept.numel())
        d_kept[kp.seen:] = 0
        _pipe_join(dv, pipe, d_kept)
        pipe.spool.put(d_kept, kp.seen, pipe.run.chunk_blocks * BLOCK)
        pipe.ledger.drop(d_kept.numel())
        del d_kept
    kp.host, kp.d_keys, kp.lens = [], [], []                    # (the spool's own key pass computes them again)


def _pipe_key_pass(dv, opened, range_bytes, kp, d_stream=None, spool_header=None):
    """key pass of a pipe, the ONLY pass over its text: per chunk -- read by the reader's thread while the device works on the chunk
    before -- upload, svx_sam_lines, svx_sam_measure, the read-back and the host's lines as :func:`_sam_key_pass` has them, and AT ONCE
    svx_sam_encode: the chunk's records into a segment of exactly their bytes, their offsets the exclusive sum of the lengths behind
    the bytes kept so far; the host's encodings copied to theirs.  What is kept is a SAM file's; :func:`_pipe_fill` joins the segments.
    A chunk that :func:`keeps_in_core` refuses (``spool_header`` given: the first) opens the spool: from then on every chunk's
    records are appended to it in arrival order and nothing is kept; ``opened.pipe.mode`` says so to the caller."""
    from .io import sam
    torch, kernels, dev, clock, pipe = dv.torch, dv.kernels, dv.dev, dv.clock, opened.pipe
    kp.reader = textin.ChunkReader(torch, dv.lib, clock)
    if spool_header is not None:
        _pipe_to_spool(dv, opened, kp, spool_header)
    d_status = torch.zeros(1, dtype=torch.int32, device=dev)
    for chunk in kp.reader.chunks(opened.text, range_bytes):
        d_text, d_line_off, n_lines = textin.upload_lines(torch, kernels, dev, clock, chunk)
        m = _sam_measured(dv, opened, kp, chunk, d_text, d_line_off, n_lines)
        need = int(m.length.sum())
        if pipe.spool is None and need and not keeps_in_core(kp.seen, need, pipe.run.budget):
            _pipe_to_spool(dv, opened, kp, sam.bam_header_bytes(opened.head))
        # ---- the chunk's records: a segment of their bytes (kept), or a buffer with the encoder's slack (spooled at once)
        off = np.cumsum(m.length) - m.length
        d_seg = torch.empty(need + (STREAM_SLACK if pipe.spool is not None else 0), dtype=torch.uint8, device=dev)
        d_seg[need:] = 0
        if n_lines:
            kernels.sam_encode(d_text, chunk.n, d_line_off, n_lines, kp.sam_table, torch.from_numpy(m.kernel_len).to(dev),
                               torch.from_numpy(off + kp.seen).to(dev), kp.seen, d_seg, d_status)
        clock.lap("encode")
        pipe.host_lines += _place_host_records(torch, kp.host_records.pop, m.kernel_len, m.first, off, d_seg)
        clock.lap("host_lines")
        if int(d_status.item()):
            raise SortWriteError("%s: a line's record is not of the length svx_sam_measure gave it" % opened.path)
        if pipe.spool is not None:
            pipe.spool.put(d_seg, need, pipe.run.chunk_blocks * BLOCK)
        elif need:
            pipe.segments.append(d_seg)
            pipe.ledger.add(need)
        _keep_measured(kp, chunk.place, m, keys=pipe.spool is None)
        del d_text, d_line_off, d_seg
        clock.lap("keep")
    opened.text.close()
    if pipe.spool is not None:
        pipe.spool_file = pipe.spool.finish()
        pipe.spool_bytes = pipe.spool.bytes


def _pipe_fill(dv, opened, kp):
    """in one piece, a pipe: its segments joined into the resident stream (``kp.d_stream``) -- both copies exist while they are."""
    opened.pipe.ledger.add(kp.d_stream.numel())
    _pipe_join(dv, opened.pipe, kp.d_stream, int(kp.off_in[0]) if kp.n else kp.base)


def _pipe_again(dv, opened, kp, need):
    raise SortWriteError("%s: a pipe cannot be read again" % opened.path)      # (not reached: a pipe beyond the budget is spooled)


def _pipe_spooled(dv, opened, header):
    """A pipe among several inputs: its text through :func:`_pipe_key_pass` into the spool file from the first byte on, under the
    merged ``header`` and in the merged numbering -> the Opened of that file, a BAM like any other."""
    _pipe_key_pass(dv, opened, opened.pipe.run.range_bytes, KeyPass(), None, header)
    return _open(opened.pipe.spool_file, alone=False)._replace(pipe=opened.pipe)


def _bam_pipe_key_pass(dv, opened, range_bytes, kp, d_stream=None):
    """key pass of a BAM on a pipe, the ONLY pass over it: :func:`_key_pass`'s body per range of index.stream_ranges -- the fields, the
    lengths, the keys, :func:`_retid` where there is a remap -- and the range's record bytes ``d_raw[first:exit_off]`` AT ONCE into a
    segment of exactly their size, as :func:`_pipe_key_pass` keeps a chunk's.  The first range :func:`keeps_in_core` refuses opens the
    spool under the stream's own header, the kept records first (:func:`_pipe_to_spool`); from then on every range's records are
    appended to it and nothing is kept; ``opened.pipe.mode`` says so to the caller."""
    torch, dev, clock, pipe = dv.torch, dv.dev, dv.clock, opened.pipe
    chunks = textin.member_chunks(torch, opened.text, range_bytes)
    for rng in index.stream_ranges(chunks, opened.head, opened.first, dev, clock, name=opened.path):
        kp.range_records.append(int(rng.n_rec))
        kp.places.append(rng.place)
        if rng.n_rec:
            tid, pos, flag, span, rec_off = index._index_fields(dv.lib, torch, dv.kernels, dev, rng, clock)
            first, last = int(rec_off[0]), int(rng.exit_off)
            need = last - first
            if opened.remap is not None:
                _retid(dv, opened, kp, rng.d_raw, rng.d_rec_off, rng.d_tid)
                tid = np.where(tid >= 0, opened.remap[np.maximum(tid, 0)], tid).astype(np.int32)
            if pipe.spool is None and not keeps_in_core(kp.seen, need, pipe.run.budget):
                _pipe_to_spool(dv, opened, kp, pipe.bam_header)
            d_seg = torch.empty(need + (STREAM_SLACK if pipe.spool is not None else 0), dtype=torch.uint8, device=dev)
            d_seg[:need].copy_(rng.d_raw[first:last])           # the records that complete in the range: contiguous there
            d_seg[need:] = 0
            if pipe.spool is not None:
                pipe.spool.put(d_seg, need, pipe.run.chunk_blocks * BLOCK)
            else:
                pipe.segments.append(d_seg)
                pipe.ledger.add(need)
                kp.host.append((tid, pos, flag, span))
                kp.lens.append(np.diff(np.append(rec_off, np.uint64(last)).astype(np.int64)))
                kp.d_keys.append((rng.d_tid, rng.d_pos))
            kp.seen += need
            del d_seg
        rng.d_raw = rng.d_starts = rng.d_base = rng.d_cigar = rng.d_cig_off = rng.d_names = rng.d_name_off = rng.d_rec_off = None
        del rng
        clock.lap("keep")
    opened.text.close()
    if pipe.spool is not None:
        pipe.spool_file = pipe.spool.finish()
        pipe.spool_bytes = pipe.spool.bytes


BAM_SOURCE = Source("bam", _key_pass, _bam_again, lambda dv, opened, kp: _bam_fill(dv, opened, kp))
BAM_PIPE_SOURCE = Source("bam_pipe", _bam_pipe_key_pass, _pipe_again, _pipe_fill)
SAM_SOURCE = Source("sam", _sam_key_pass, _sam_again, lambda dv, opened, kp: _sam_fill(dv, opened, kp))     # (looked up at the call: tests replace it)
PIPE_SOURCE = Source("pipe", _pipe_key_pass, _pipe_again, _pipe_fill)


def _bai(opened, kp, od, written, fmt="bai"):
    """index: the ``.bai`` (``fmt="csi"``: the ``.csi``) of the written file, from the sorted fields and the writer's ledger -> its bytes."""
    from .io import bai
    voff = bai.virtual_offsets(written.dst, written.coff, (od.off_out + len(opened.header)).astype(np.uint64))
    order = od.order
    tid, pos, flag, span = kp.tid[order], kp.pos[order].astype(np.int64), kp.flag[order], kp.span[order].astype(np.int64)
    try:
        return index.index_bytes(fmt, 14, opened.head, tid, pos, pos + np.maximum(span, 1), flag, voff[:-1], voff[1:])
    except bai.TooLong as exc:
        raise SortWriteError("%s: %s" % (opened.path, index.too_long_message(exc, opened.head.references, "write a .csi instead: --csi "
                                                                            "(SVX_SORT_INDEX=csi; sort_bam's index_format)"))) from None
    except ValueError as exc:
        raise SortWriteError("%s: %s" % (opened.path, exc)) from None


def sort_bam(bam_path, out_path, device="cuda", range_bytes=None, chunk_bytes=None, stats=None, tables="fixed", memory_bytes=None,
             index_format="bai", pipe_bam=None):
    """Write the records of ``bam_path`` in coordinate order to ``out_path`` and its index to ``out_path + ".bai"`` (see the head of the
    module); returns ``out_path``.  ``index_format="csi"``: the index is ``out_path + ".csi"`` and no ``.bai`` is written -- the sorted file's
    bytes are the same.  Under "bai" a record that reaches position 2^29 is refused (SortWriteError, neither file written): a ``.bai``
    cannot address it, and the format is never switched without being asked.  ``range_bytes``: compressed bytes a range of the pass (default: the device decoder's group size),
    ``chunk_bytes``: inflated bytes a chunk of the output (default DEFAULT_CHUNK_BYTES; whole blocks, at least one) -- tests pass small
    values.  ``tables``: "fixed" -- every block in the fixed Huffman code or stored -- or "dynamic": Huffman codes built per block where
    they are smaller; the inflated bytes and the index's records are the same.  ``memory_bytes``: the budget for the records' inflated
    bytes on the device (default: half of the device memory that is free at the call); a file whose records exceed it is written in
    spans, a pass over the input for each (see the head of the module) -- the same two files.  ``stats``: a dict that receives
    ranges, records, blocks, stored_blocks, dynamic_blocks, compressed_bytes, inflated_bytes, chunks, spans (1: in one piece),
    span_range_reads (ranges read again over all spans; 0 in one piece), range_records (the records every range of the pass
    completed), stream_bytes (the largest record buffer allocated), inputs, input_records (the records of every input), retid_inputs
    (the inputs whose records were renumbered: svx_record_retid) and the seconds per stage.  ``bam_path`` may be SAM text: then
    ``range_bytes`` is the text bytes of a chunk, and stats also has input="sam" and host_lines, the lines io/sam.py encoded.
    ``bam_path`` may be a list or tuple of such paths: their records merged into the one sorted file (see "Several inputs" at the head
    of the module); ranges and range_records run over all inputs in list order, host_lines is there when a part is SAM text, input only
    when all are; a list of one path is that path, an empty one a ValueError.  ``-`` (standard input) or a path that is no regular file
    is read once (see "A pipe" at the head of the module): stats also has ``pipe`` -- mode, grows, spool_bytes, text_bytes and the
    reader thread's waits; ``pipes``: the same of every such input in list order, with its name --, input="sam" as for a SAM file, and
    stream_bytes is the largest total of the pipe's record buffers.  A side effect on the calling PROCESS: when the call fails while
    ``-`` is among the inputs, descriptor 0 is pointed at the null device (textin.TextInput.close) before the error is raised -- that closes the
    pipe's read end, so that its writer ends with EPIPE and does not block; a caller that needs standard input afterwards hands the
    stream in as a path (/dev/fd/N of a duplicate) instead, whose descriptor is the call's own.  ``pipe_bam``: what becomes of a BAM
    that arrives on a pipe -- "spool" (the default): copied as it is into a file beside the output and sorted from there; "stream": a
    lone such pipe is taken in one pass, ``range_bytes`` compressed bytes a chunk (default textin.DEFAULT_PIPE_BAM_BYTES), and
    ``stats["pipe"]`` has mode "in_core" or "spooled", holds="bam" and compressed_bytes; None: ``SVX_PIPE_BAM`` of the environment."""
    from . import ingest_sort, kernels
    paths = input_paths(bam_path)
    torch, lib, dev, clock = index.on_device("sort_bam needs the GPU (svx_record_sort, svx_bgzf_deflate)", device, STAGES)
    if tables not in TABLES:
        raise ValueError("tables: %r is none of %s" % (tables, ", ".join(TABLES)))
    if index_format not in index.FORMATS:
        raise ValueError("index_format: %r is none of %s" % (index_format, ", ".join(index.FORMATS)))
    stream_bam = textin.pipe_bam_setting(pipe_bam, "sort_bam")
    dv = _Dev(torch, lib, kernels, dev, clock)
    chunk_blocks = max(int(chunk_bytes or DEFAULT_CHUNK_BYTES) // BLOCK, 1)
    budget = None if memory_bytes is None else max(int(memory_bytes), 1)
    ins, opened, kp, writer, counts, pipes, done = None, None, KeyPass(), None, {"span_range_reads": 0}, [], False
    first_name = textin.name_of(paths[0])
    bam_path = first_name if len(paths) == 1 else "%s (+ %d more)" % (first_name, len(paths) - 1)       # (the inputs' name in a message)
    try:
        with torch.cuda.device(dev):
            if budget is None:                                  # half of what is free: the rest is for a range, its inflate workspace, keys and chunks
                budget = max(int(torch.cuda.mem_get_info(dev)[0]) // 2, 1)
            ins = _open_all(paths, dv, _Run(out_path, chunk_blocks, budget, range_bytes, pipes, clock, stream_bam))
            opened = ins.merged
            opened, kp, spanned = _key_passes(dv, ins, budget, range_bytes)
            od = _order(dv, opened, kp, spanned, budget)
            pieces = _pieces_spanned if spanned else _pieces_in_core
            writer = BgzfWriter(out_path, DeviceEncode(dv, tables), clock, bam_path)
            writer.put_header(torch.from_numpy(np.frombuffer(opened.header, np.uint8).copy()).to(dev), len(opened.header))
            for piece in pieces(dv, opened, kp, od, chunk_blocks, counts):
                writer.put(*piece)
                del piece                                       # (the chunk's buffer goes before the generator allocates the next)
            written = writer.finish()
            commit_pair(writer.tmp, out_path, _bai(opened, kp, od, written, index_format), "." + index_format)
            clock.lap("index", False)
            done = True
    except index.IndexBuildError as exc:
        raise SortWriteError("%s: %s" % (kp.reading or bam_path, exc)) from None
    except torch.cuda.OutOfMemoryError as exc:
        raise SortWriteError("%s: the device has no room for the file's records -- %d inflated record bytes in all, %d seen so far, a budget of "
                             "%s bytes for them; a smaller one (--memory, SVX_SORT_MEMORY; sort_bam's memory_bytes) writes the file in more "
                             "spans (%s)" % (bam_path, kp.seen if opened is None or opened.room is None else opened.room, kp.seen, budget,
                                             str(exc).split("\n")[0])) from None
    except _lib.SvxError as exc:
        raise SortWriteError("%s: %s" % (kp.reading or bam_path, exc)) from None
    except textin.ReadError as exc:
        raise SortWriteError(str(exc)) from None
    except OSError as exc:
        raise SortWriteError("%s: writing %s failed (%s)" % (bam_path, out_path, exc)) from None
    finally:
        for pipe in pipes:                                      # the read end first: the pipe's writer must not block on it
            pipe.input.close(failed=not done)
        if writer is not None:
            writer.discard()
        for pipe in pipes:
            pipe.discard()
    if stats is not None:
        was_text = lambda o: o.source is SAM_SOURCE or o.pipe is not None and o.pipe.holds == "sam"
        sam_parts = [(o, part) for o, part, _r, _n in kp.parts if was_text(o)]
        if sam_parts:
            stats.update(host_lines=sum(len(part.host_records) if o.pipe is None else o.pipe.host_lines for o, part in sam_parts))
            if len(sam_parts) == len(kp.parts):
                stats.update(input="sam")
        if pipes:
            # ``pipe``: the first input that was read once; ``pipes``: every one of them, in list order, with its name
            stats.update(pipe=pipes[0].stats(), pipes=[dict(pipe.stats(), name=pipe.name) for pipe in pipes])
        stats.update(inputs=len(kp.parts), input_records=[part.n for _o, part, _r, _n in kp.parts],
                     retid_inputs=sum(o.remap is not None for o, _part, _r, _n in kp.parts))
        stats.update(ranges=len(kp.range_records), records=kp.n, blocks=written.blocks, stored_blocks=written.stored_blocks,
                     dynamic_blocks=written.dynamic_blocks, chunks=written.chunks, spans=od.spans, span_range_reads=counts["span_range_reads"],
                     range_records=kp.range_records, stream_bytes=max([od.stream_bytes] + [pipe.ledger.peak for pipe in pipes]), memory_bytes=budget,
                     compressed_bytes=written.compressed_bytes, inflated_bytes=written.inflated_bytes, pos_bits=od.pos_bits,
                     passes=len(ingest_sort.digit_plan(len(opened.head.references), od.pos_bits)),
                     seconds={k: round(v, 6) for k, v in clock.times.items()})
    return out_path


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(prog="python -m svision_amd.sort", description="Write the coordinate-sorted BAM of an unsorted BAM or of SAM text, and its .bai, on the GPU.")
    ap.add_argument("bam", nargs="+", help="an unsorted BAM or SAM text; several: their records merged into the one sorted file.  ``-`` (once) is "
                                           "standard input, and a path that is no regular file (a FIFO, /dev/fd/N) is read once like it: an aligner's "
                                           "output through a pipe")
    ap.add_argument("-o", "--output", required=True, help="the sorted BAM to write (its index: OUTPUT + .bai, with --csi OUTPUT + .csi)")
    ap.add_argument("-c", "--csi", action="store_true", default=os.environ.get("SVX_SORT_INDEX") == "csi",
                    help="write the index as a .csi: the format for references with positions from 2^29 on (default: $SVX_SORT_INDEX=csi)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--chunk-bytes", type=int, default=None, help="inflated bytes a chunk of the output (default %d)" % DEFAULT_CHUNK_BYTES)
    ap.add_argument("--tables", choices=TABLES, default=os.environ.get("SVX_SORT_TABLES") or "fixed",
                    help="the encoder's Huffman codes: fixed, or built per block where that is smaller (default: $SVX_SORT_TABLES, or fixed)")
    ap.add_argument("--memory", type=parse_memory, default=os.environ.get("SVX_SORT_MEMORY") or None, metavar="BYTES",
                    help="device memory for the records' inflated bytes, with an optional K, M or G; a file with more is written in spans, a "
                         "pass over the input for each (default: $SVX_SORT_MEMORY, or half of the device memory that is free)")
    ap.add_argument("--pipe-bam", choices=textin.PIPE_BAM, default=os.environ.get("SVX_PIPE_BAM") or "spool",
                    help="a BAM that arrives on a pipe (dorado aligner, pbmm2): spool -- copied into a file beside the output, then sorted -- or "
                         "stream -- a lone one taken in one pass, no file in between (default: $SVX_PIPE_BAM, or spool)")
    ap.add_argument("--stats-json", default=None, help="also write the statistics to this file")
    args = ap.parse_args(argv)
    if args.tables not in TABLES:
        ap.error("SVX_SORT_TABLES=%s: fixed or dynamic" % args.tables)
    if args.pipe_bam not in textin.PIPE_BAM + ("0",):
        ap.error("SVX_PIPE_BAM=%s: spool or stream" % args.pipe_bam)
    if os.environ.get("SVX_SORT_INDEX") not in (None, "", "bai", "csi"):
        ap.error("SVX_SORT_INDEX=%s: bai or csi" % os.environ["SVX_SORT_INDEX"])
    stats = {}
    try:
        path = sort_bam(args.bam[0] if len(args.bam) == 1 else args.bam, args.output, device=args.device, chunk_bytes=args.chunk_bytes, stats=stats, tables=args.tables,
                        memory_bytes=args.memory, pipe_bam=args.pipe_bam, **(dict(index_format="csi") if args.csi else {}))
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
    if "pipe" in stats:
        pipe = stats["pipe"]
        name = next((textin.name_of(b) for b in args.bam if is_stream(b)), "<stdin>")
        print("%s: %s (%d bytes%s) %s" % (path, name, pipe["text_bytes"], " of BAM, taken in one pass" if pipe["holds"] == "bam" and pipe["mode"] != "bam_spooled" else "",
                                        "kept in core: its records grew %d time(s) on the device" % pipe["grows"] if pipe["mode"] == "in_core" else
                                        "spooled: %d bytes of unsorted BAM beside the output, sorted from there%s"
                                        % (pipe["spool_bytes"], " (a BAM on a pipe is copied as it is)" if pipe["mode"] == "bam_spooled" else "")))
    if len(args.bam) > 1:
        print("%s: %d inputs merged (records: %s), %d of them renumbered into the merged reference dictionary"
              % (path, len(args.bam), ", ".join(str(v) for v in stats.get("input_records", [])), stats.get("retid_inputs", 0)))
    if stats.get("spans", 1) > 1:
        print("%s: the records exceed the budget of %d bytes (--memory): written in %d span(s), %d range(s) read again"
              % (path, stats["memory_bytes"], stats["spans"], stats["span_range_reads"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
