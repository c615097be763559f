"""Write the coordinate-sorted BAM of an unsorted one -- or of SAM text --, and its ``.bai``, on the device: ``python -m svision_amd.sort in.bam -o out.bam``.

``SVX_DEVICE_SORT=1`` (svision_amd/ingest_sort.py) computes the order of an aligner's output and throws it away with the process.
Here the order becomes a file -- a standard BAM with a standard index that the default path, any number of ranks, a second caller
and a genome browser read --, with every record byte kept: qualities and aux tags too, which the packed tables drop.  The pass:

  pass      the whole file in ranges: per range tid and pos on the device, the fields and the records' lengths on the host, and the
            BYTES of the records that complete in the range (sort_sources.BamSource)
  join      the slices end to end are one record stream with CSR offsets (:func:`_join`)
  sort      ONE svx_record_sort, the key and the stability of SVX_DEVICE_SORT=1: (reference, position), no reference last, ties in
            file order (:func:`_order`)
  output    the output stream cut every 0xFF00 bytes and taken in chunks: gathered (:func:`_pieces_in_core`), deflated, packed,
            downloaded and appended to a temporary file (the head of sort_out.py)
  header    the input's header with its @HD line set to SO:coordinate, in blocks of its own (the head of sort_header.py)
  index     svision_amd.io.bai.bai_bytes on the sorted fields, end = pos + max(span, 1), the virtual offsets from the records' stream
            offsets, the 0xFF00 cut and the prefix of the members' lengths; both files are renamed into place together
            (``index_format="csi"`` / ``--csi`` / ``SVX_SORT_INDEX=csi``: io.csi.csi_bytes and ``.csi``; a record that reaches position
            2^29 is refused under the default ``.bai``, and neither file is left)

Device memory: the records' inflated bytes once -- or a span of them, see below -- (the stream is allocated before the pass, sized by
the sum of the BGZF members' ISIZE fields, and every range's slice is copied straight into it), one range of the pass, 8 bytes of key + 20 of sort workspace a
record, and one chunk (the head of sort_out.py).

A file larger than the device.  The records' bytes are what may not fit: keys, ranks and offsets are about 50 bytes a record.
``memory_bytes`` (``--memory BYTES`` with K / M / G, ``SVX_SORT_MEMORY``; default: half of the device memory that is free at the call --
the other half is for a range, its inflate workspace, keys and chunk buffers; a first guess, see profiles/sort_spans.txt) is the budget
for them.  Records that fit take the path above, unchanged.  Otherwise the order is still computed in ONE sort and only the bytes are
placed in pieces, the same two files byte for byte:

  key pass  the pass above keeping no record byte (sort_sources.BamSource)
  sort      the same svx_record_sort and svx_record_gather_offsets; svx_record_invert gives every input record its rank
  plan      :func:`plan_spans` cuts the output's record stream every ``max(memory_bytes // 0xFF00, 1)`` blocks -- whole blocks, so the
            0xFF00 cuts fall where they fall in one piece.  A span's buffer holds every record that touches the span whole: a record
            across an edge is placed in both neighbours' buffers, a buffer exceeds the span by less than two records
  span pass per span, the ranges that own a record of it (:func:`span_ranges`) and no others are read again and scattered to their
            output offsets in the span's buffer (:func:`_pieces_spanned`; the source's ``again``)
  output    the span's buffer through the chunk loop without the gather, ``chunk_bytes`` capped at the span

The roads of the other inputs, each described where it is implemented, in svision_amd/sort_sources.py: SAM text (``SamSource``); a pipe
(``_Pipe``, ``_open_pipe``), its one pass (``PipeSource.key_pass``), how its stream grows and the spool beyond the budget
(``PipeStore``), among several inputs (``_pipe_spooled``), a BAM on a pipe (``_open_pipe``) and streamed (``BamPipeSource``).

Several inputs.  ``sort_bam([a.bam, b.sam, c.bam], out)`` -- ``python -m svision_amd.sort a.bam b.sam c.bam -o out.bam`` -- writes ONE sorted
BAM of all their records, what ``samtools merge`` in front of the sort would have given: one BAM per SMRT cell, one SAM per FASTQ batch.
The two files are, byte for byte, those of ONE unsorted BAM that holds the merged header and the inputs' records one input after the
other, every reference index in the merged numbering; ties of (reference, position) therefore come out in list order, then file order:
the stability of the one svx_record_sort over the inputs' keys end to end.

  open      every input as above; sort_header.merge_headers (host, its rules stand there) gives the output's text, its dictionary -- the
            union of the inputs' by name, in order of first appearance -- and per input the table old refID -> merged refID (:func:`_open_all`)
  key pass  input by input in list order, each with its own header, first record and ranges; a BAM whose table is not the identity is
            renumbered where its records lie, SAM text is measured against the merged names (sort_sources.BamSource, SamSource)
  join      ranges, keys and offsets of all inputs end to end: ``ranges`` and ``range_records`` of the statistics run over all of them
  spans     a span's ranges are read again input by input (the source's ``again``), a BAM's records translated again before the scatter
  retag     (``retag``, off by default) @RG / @PG IDs that collide are renamed in the merged header and the RG:Z / PG:Z values of that
            input's records rewritten, a wave a record (sort_sources._retag); its record bytes are then known only behind its key
            pass, so the run takes the road of a mixed run below and reads its BAM inputs twice
  room      all inputs BAM: the sum of their ISIZE-derived rooms is known before the passes, the stream is allocated once, as for one
            file.  With SAM text among them the records' bytes are known only behind the key passes; they keep no byte, and a run
            that fits then fills the stream input by input (the source's ``fill``; :func:`_key_passes`)
A failure names the input it came from; "changed while it was sorted" names the input that changed.

Optional fields removed.  ``drop_tags`` / ``keep_tags`` (``--drop-tags fi,fp,ri,rp``, ``--keep-tags RG,NM,SA,MD``; ``SVX_SORT_DROP_TAGS`` /
``SVX_SORT_KEEP_TAGS``; off by default) remove optional fields from every record as it is sorted -- the kinetics arrays, base
modifications and move tables that pbmm2 and dorado carry over from unaligned BAMs and that are often most of a record.  The two files
are, byte for byte, those of the same inputs whose records had those fields removed beforehand (:func:`tag_filter` has the rules;
``CG`` always stays).  A wave a record on the device (sort_sources._tags), in the key pass and again per range of a span.  Records only
get shorter, so ``room`` stays the ISIZE sum: the stream is allocated once, the shortened records are kept as the key passes go, and no
input is read twice; whether the file is written in spans is decided on the unfiltered size.  An input read as SAM text is refused
under the switch, and a lone BAM on a pipe is sorted from its spool copy under either ``pipe_bam``.

A corrupt block, a CRC mismatch, a malformed or cut chain, a device allocation or a write that fails raises SortWriteError (a
ValueError); no file and no temporary is left behind.

:func:`sort_bam` is the list of its steps, each a function of this module over named values: ``_open_all`` (per input
sort_sources._open, which also chooses the input's source: a BAM, SAM text or a pipe; several inputs: sort_header.merge_headers) ->
``_key_passes`` (per input its source's key pass into its own sort_sources.InputPass; a pipe that was spooled is opened again as its
spool file; then ``_join`` into the run's :class:`RunPass`; where the records' size was not known before, the sources' ``fill``) ->
``_order`` -> the pieces, ``_pieces_in_core`` or ``_pieces_spanned``: generators of (device buffer, first byte, bytes), a chunk each ->
sort_out.BgzfWriter -> ``_bai`` -> sort_out.commit_pair -> ``_stats``.  Which records a chunk or a span takes is one rule,
:func:`records_touching`.  The names of the other modules that callers use are imported below and stay reachable here.
"""
import collections
import os
import re
import sys

import numpy as np

from . import _lib, index, textin
from .sort_header import MergedHeader, SortWriteError, merge_headers, sorted_header_bytes, sorted_header_text     # noqa: F401  (their names here are in use)
from .sort_out import BLOCK, DEFAULT_CHUNK_BYTES, STREAM_SLACK, BgzfWriter, DeviceEncode, Spool, _Dev, block_cuts, chunk_cuts, commit_pair, spool_copy, spool_path   # noqa: F401
from .sort_sources import Opened, PipeStore, SamSource, StreamLedger, TagFilter, _open, _pipe_spooled, _rec_base, _Run, inflated_size, keeps_in_core   # noqa: F401
from .textin import DEFAULT_SAM_CHUNK_BYTES, SAM_READ_THREADS, input_paths, is_stream    # noqa: F401

TABLES = ("fixed", "dynamic")                                   # the encoder: svx_bgzf_deflate / svx_bgzf_deflate_dyn
STAGES = ("read", "upload", "inflate", "crc", "find_starts", "walk", "scan", "read_back", "keep", "join", "sort", "gather", "scatter", "deflate",
          "pack", "download", "write", "index", "lines", "measure", "encode", "host_lines", "retid", "spool", "retag", "tags")


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


_TAG = re.compile(r"[A-Za-z][A-Za-z0-9]\Z")
TAGS_ALWAYS_KEPT = "CG"             # the real CIGAR of a record with more than 65,535 operations


def parse_tags(value, name):
    """A list of optional-field tags -- a list or tuple of 2-character strings, or ONE comma-separated string ("" is the empty list)
    -> a tuple of them.  A tag is ``[A-Za-z][A-Za-z0-9]``; anything else, or a tag that is listed twice: ValueError, naming ``name``."""
    if isinstance(value, str):
        items = value.split(",") if value.strip() else []
    elif isinstance(value, (list, tuple)):
        items = list(value)
    else:
        raise ValueError("%s: a list of tags or one comma-separated string, not %r" % (name, value))
    for tag in items:
        if not isinstance(tag, str) or not _TAG.match(tag):
            raise ValueError("%s: %r is no tag -- a letter followed by a letter or a digit (fi, MM, X0)" % (name, tag))
    twice = sorted({tag for tag in items if items.count(tag) > 1})
    if twice:
        raise ValueError("%s: %s is listed twice" % (name, ", ".join(twice)))
    return tuple(items)


def tag_filter(drop_tags=None, keep_tags=None, environ=None):
    """sort_bam's ``drop_tags`` / ``keep_tags`` -> the run's TagFilter(mode, tags), or None: off.

      drop_tags  every optional field whose two-byte tag is listed is removed, whatever its type and however often it occurs; an
                 empty list removes nothing: off
      keep_tags  every field whose tag is NOT listed is removed; an empty list removes all fields
      CG         is never removed: it holds the real CIGAR of a record with more than 65,535 operations.  Naming it in ``drop_tags``
                 is an error, and every keep list implies it
    The two exclude each other.  Both None: ``SVX_SORT_DROP_TAGS`` / ``SVX_SORT_KEEP_TAGS`` of ``environ`` (os.environ) are read, comma-
    separated, an empty value being unset; an argument that is given wins over the environment.  Errors are ValueError."""
    names = ("drop_tags", "keep_tags")
    if drop_tags is None and keep_tags is None:
        environ = os.environ if environ is None else environ
        drop_tags, keep_tags = (environ.get(name) or None for name in ("SVX_SORT_DROP_TAGS", "SVX_SORT_KEEP_TAGS"))
        names = ("SVX_SORT_DROP_TAGS", "SVX_SORT_KEEP_TAGS")
    if drop_tags is not None and keep_tags is not None:
        raise ValueError("%s and %s exclude each other: a list to drop, or a list to keep" % names)
    if drop_tags is not None:
        tags = parse_tags(drop_tags, names[0])
        if TAGS_ALWAYS_KEPT in tags:
            raise ValueError("%s: %s is never removed -- it holds the CIGAR of a record with more than 65,535 operations" % (names[0], TAGS_ALWAYS_KEPT))
        return TagFilter("drop", tags) if tags else None
    if keep_tags is not None:
        return TagFilter("keep", parse_tags(keep_tags, names[1]))
    return None


# ---- the steps ----
# Every input opened, and the one file they make: ``merged`` is an Opened whose head (references, lengths), header bytes and room are
# the output's -- of one input: that input's own --, ``label`` names the inputs in a message.
Inputs = collections.namedtuple("Inputs", "opened merged label")
MergedHead = collections.namedtuple("MergedHead", "references lengths")
# One input of the run: its Opened, its own pass (a sort_sources.InputPass), the number of its first range and of its first record in the run.
Part = collections.namedtuple("Part", "opened part first_range first_record")


class RunPass:
    """What the key passes over all inputs leave for the run, joined (:func:`_join`): ``range_records`` and ``places`` per range, over
    all inputs; ``seen``: the inflated record bytes; the ``n`` records' host fields ``tid pos flag span``, the device keys ``d_tid d_pos``
    (until the sort has taken them), the records' offsets in the joined stream ``off_in`` / ``d_off_in`` [n + 1], and ``d_stream``: the
    resident record stream, None in a spanned run.  ``parts``: a :class:`Part` per input, whose own pass has its ranges and its slices
    of the offsets.  ``reading``: the input that is being read, for a failure's message."""

    def __init__(self):
        self.range_records, self.places, self.seen, self.n, self.parts, self.reading = [], [], 0, 0, [], None
        self.tid = self.pos = self.flag = self.span = self.d_tid = self.d_pos = self.off_in = self.d_off_in = self.d_stream = None


def _open_all(paths, dv=None, run=None):
    """open, every input: -> Inputs.  One input: as it is opened.  Several: the headers merged (:func:`merge_headers`) -- a SAM part
    takes the merged dictionary for its own, so its records are encoded in the merged numbering and a part without header is
    usable; a BAM part whose table is not the identity carries it as ``remap`` --, ``room`` the sum where every part's is known.
    Under ``run.retag`` a BAM part whose @RG / @PG IDs were renamed carries its table as ``retag``: its records change their length, so
    the run's ``room`` is None -- the road of a mixed BAM + SAM run; the part's own ``room`` stays its ISIZE sum, for the check of the
    bytes as read.  A part read as text that would need a rename is refused.  Under ``run.tags`` every part carries the filter as
    ``tags``; its records only get shorter, so every ``room`` stays the ISIZE sum -- an upper bound --, and a part read as text is
    refused: text is encoded straight into the resident stream."""
    from .io import sam
    if paths.count("-") > 1:
        raise SortWriteError("%s is named twice: standard input is one stream" % sam.STREAM_NAME)
    tags = None if run is None else run.tags

    def filtered(o):
        if tags is None:
            return o
        if o.source.from_text:                                  # (before a pipe among them is spooled)
            raise SortWriteError("%s: the input is read as SAM text, whose records' optional fields are not filtered (--%s-tags, SVX_SORT_%s_TAGS; "
                                 "sort_bam's %s_tags) -- convert it to BAM (`samtools view -b`, also in a pipe)"
                                 % (o.path, tags.mode, tags.mode.upper(), tags.mode))
        return o._replace(tags=tags)
    if len(paths) == 1:
        opened = filtered(_open(paths[0], run=run))
        return Inputs([opened], opened, opened.path if opened.pipe is None else opened.pipe.name)
    opened = [filtered(_open(p, alone=False, run=run)) for p in paths]
    merged = merge_headers([(o.path, o.head.text if o.source.from_text else o.head.header_text, o.head.references, o.head.lengths) for o in opened],
                           retag=bool(run is not None and run.retag))
    for o, table in zip(opened, merged.renames):
        if table and o.source.from_text:                        # (before a pipe among them is spooled)
            (tag, old), new = next(iter(table.items()))
            raise SortWriteError("%s: its @%s ID %s is on another line in an earlier input and would become %s, but the input is read as SAM "
                                 "text, whose records' %s:Z tags are not rewritten -- list %s first: the first input to bring an ID keeps "
                                 "it (or convert it to BAM)" % (o.path, tag, old.decode("latin-1"), new.decode("latin-1"), tag, o.path))
    header = sam.bam_header_bytes(sam.SamHead(merged.references, merged.lengths, merged.text, "coordinate"))
    for i, o in enumerate(opened):
        if o.source.from_text:                                  # text: measured and encoded against the merged names
            opened[i] = o = o._replace(head=sam.SamHead(merged.references, merged.lengths, o.head.text, o.head.sort_order))
            if o.source.reads_once:                             # a pipe among several: spooled from its first byte, under the merged header
                opened[i] = _pipe_spooled(dv, o, header)
        elif not np.array_equal(merged.maps[i], np.arange(len(merged.maps[i]))):       # (a dictionary that opens the merged one: nothing to rewrite)
            opened[i] = o = o._replace(remap=merged.maps[i])
        if merged.renames[i]:                                   # (a BAM: text was refused above)
            opened[i] = o._replace(retag=merged.renames[i])
    # an input whose records are rewritten has its record bytes only behind its key pass: the run's room is not known before
    rooms = [None if o.retag else o.room for o in opened]
    label = "%s (+ %d more)" % (paths[0], len(paths) - 1)
    return Inputs(opened, Opened(label, MergedHead(merged.references, merged.lengths), None, header,
                                 None if None in rooms else sum(rooms), None), label)


def _pass_each(dv, ins, budget, range_bytes):
    """Every input's key pass, in list order -> the run's RunPass, its parts filled and not yet joined.  Where every input's ``room`` is
    known before (BAMs: the ISIZE sums) and fits the budget, the stream is allocated first and the records are kept as the passes go."""
    kp, room = RunPass(), ins.merged.room
    if room is not None and room <= budget:
        kp.d_stream = dv.torch.empty(room + 4, dtype=dv.torch.uint8, device=dv.dev)   # (4 readable bytes behind it: the gather's aligned loads)
    ranges = records = 0
    for opened in ins.opened:
        part = opened.source.state(kp.seen)
        kp.parts.append(Part(opened, part, ranges, records))
        kp.reading = opened.path
        opened.source.key_pass(dv, opened, range_bytes, part, kp.d_stream)
        kp.seen += part.seen
        ranges, records = ranges + len(part.range_records), records + sum(part.range_records)
    kp.reading = None
    return kp


def _key_passes(dv, ins, budget, range_bytes):
    """key pass, every input in list order -> (the merged Opened with its ``room`` known, the run's RunPass joined, ``spanned``).  Where
    every input's ``room`` is known before, the records are kept as the passes go wherever they fit the budget; where they do not
    fit, no byte is kept in the pass and the output is filled in spans.  A lone pipe that did not fit lies in its spool file behind its
    pass: what the pass kept is dropped, the input becomes that file and takes the road of a BAM, its passes run over it.
    With SAM text among the inputs ``room`` is exact only behind the passes: they keep no byte, and a run that fits then fills the
    stream input by input (the source's ``fill``: the text encoded, a BAM's ranges read a second time, one copy a range)."""
    kp = _pass_each(dv, ins, budget, range_bytes)
    lone = ins.opened[0]
    if lone.source.reads_once and lone.pipe.store.mode == "spooled":
        del kp
        again = _open(lone.pipe.store.spool_file)._replace(pipe=lone.pipe)
        ins = Inputs([again], again, ins.label)
        kp = _pass_each(dv, ins, budget, None)
    merged = ins.merged
    known = merged.room is not None
    _join(dv, merged, kp)
    if not known:
        merged = merged._replace(room=int(kp.off_in[-1]))
    spanned = merged.room > budget
    if not known and not spanned:
        kp.d_stream = dv.torch.empty(merged.room + 4, dtype=dv.torch.uint8, device=dv.dev)
        kp.d_stream[merged.room:] = 0
        for p in kp.parts:
            kp.reading, p.part.d_stream = p.opened.path, kp.d_stream
            p.opened.source.fill(dv, p.opened, p.part)
        kp.reading = None
    return merged, kp, spanned


def _join(dv, opened, kp, cat=None, to_device=None):
    """join: what the inputs' ranges left -- per range the host fields, the device keys and the records' lengths -> ``kp``'s arrays of
    the one record stream, and every input's slices of the offsets (views: an input's pass owns no copy).  ``cat`` / ``to_device``:
    torch.cat and the upload of a host array, unless a test hands in NumPy's."""
    torch, dev, clock = dv.torch, dv.dev, dv.clock
    cat, to_device = cat or torch.cat, to_device or (lambda a: torch.from_numpy(a).to(dev))
    host, d_keys, lens = ([v for p in kp.parts for v in getattr(p.part, name)] for name in ("host", "d_keys", "lens"))
    kp.range_records = [v for p in kp.parts for v in p.part.range_records]
    kp.places = [v for p in kp.parts for v in p.part.places]
    n = kp.n = int(sum(l.size for l in lens))
    if n > 0xFFFFFFFF:
        raise SortWriteError("%s: %d records -- svx_record_sort takes up to 2^32 - 1" % (opened.path, n))
    # ---- join: CSR offsets and the keys of the one record stream
    if kp.d_stream is not None:
        kp.d_stream[kp.seen:] = 0
    kp.off_in = np.zeros(n + 1, np.int64)
    if n:
        kp.off_in[1:] = np.cumsum(np.concatenate(lens))
    kp.d_off_in = to_device(kp.off_in)
    if n:
        kp.d_tid, kp.d_pos = cat([k[0] for k in d_keys]), cat([k[1] for k in d_keys])
        kp.tid, kp.pos, kp.flag, kp.span = (np.concatenate([h[i] for h in host]) for i in range(4))
    else:
        kp.d_tid = kp.d_pos = to_device(np.empty(0, np.int32))
        kp.tid = kp.pos = kp.span = np.empty(0, np.int32)
        kp.flag = np.empty(0, np.uint16)
    del d_keys, host, lens
    for p in kp.parts:
        part, first = p.part, p.first_record
        part.n = int(sum(part.range_records))
        part.off_in, part.d_off_in = kp.off_in[first:first + part.n + 1], kp.d_off_in[first:first + part.n + 1]
        part.drop_keys()
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
    (``counts["span_range_reads"]`` of them in all; the source reads them again: its ``again``) and then given chunk by chunk -> as
    :func:`_pieces_in_core`."""
    torch, lib, kernels, dev, clock = dv
    rec_base = _rec_base(kp)
    for sp in od.plan:
        d_span = torch.empty(sp.size, dtype=torch.uint8, device=dev)
        need = span_ranges(od.rank, kp.range_records, sp.r_lo, sp.r_hi)
        clock.lap("scatter")
        for p in kp.parts:                                      # input by input: each reads its own ranges again
            mine = need[(need >= p.first_range) & (need < p.first_range + len(p.part.range_records))] - p.first_range
            d_status = torch.zeros(1, dtype=torch.int32, device=dev)
            kp.reading = p.opened.path
            for k_own, n_rec, d_raw, d_src_off in p.opened.source.again(dv, p.opened, p.part, mine) if mine.size else ():
                k = p.first_range + int(k_own)
                counts["span_range_reads"] += 1
                if n_rec != kp.range_records[k]:
                    raise SortWriteError("%s changed while it was sorted: %d records complete in the range at file offset %d, %d did in the "
                                         "first pass" % (p.opened.path, n_rec, kp.places[k][0], kp.range_records[k]))
                kernels.record_scatter_segments(d_raw, d_src_off, od.d_rank[int(rec_base[k]):int(rec_base[k + 1])], sp.r_lo, sp.r_hi,
                                                od.d_off_out, sp.base, d_span, d_status)
                clock.lap("scatter")
                del d_raw, d_src_off
            if mine.size and int(d_status.item()):
                raise SortWriteError("%s changed while it was sorted: a record's length is not the one the first pass saw" % p.opened.path)
        kp.reading = None
        for lo, hi in chunk_cuts(sp.lo, sp.hi, chunk_blocks * BLOCK):
            yield d_span, lo - sp.base, hi - lo
        del d_span


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


def _stats(stats, opened, kp, od, written, counts, pipes, budget, clock):
    """The statistics of a finished run into ``stats`` (:func:`sort_bam` names them)."""
    from . import ingest_sort
    sam_parts = [p for p in kp.parts if p.opened.source.from_text or p.opened.pipe is not None and p.opened.pipe.holds == "sam"]
    if sam_parts:
        stats.update(host_lines=sum(len(p.part.host_records) if p.opened.pipe is None else p.opened.pipe.host_lines for p in sam_parts))
        if len(sam_parts) == len(kp.parts):
            stats.update(input="sam")
    if pipes:
        # ``pipe``: the first input that was read once; ``pipes``: every one of them, in list order, with its name
        stats.update(pipe=pipes[0].stats(), pipes=[dict(pipe.stats(), name=pipe.name) for pipe in pipes])
    stats.update(inputs=len(kp.parts), input_records=[p.part.n for p in kp.parts], retid_inputs=sum(p.opened.remap is not None for p in kp.parts),
                 retag_inputs=sum(p.opened.retag is not None for p in kp.parts), retag_records=sum(getattr(p.part, "retag_records", 0) for p in kp.parts),
                 tags_mode=next((p.opened.tags.mode for p in kp.parts if p.opened.tags is not None), None),
                 tags_records=sum(getattr(p.part, "tags_records", 0) for p in kp.parts), tags_bytes=sum(getattr(p.part, "tags_bytes", 0) for p in kp.parts))
    stats.update(range_reads=sum(p.part.range_reads for p in kp.parts))
    stats.update(ranges=len(kp.range_records), records=kp.n, blocks=written.blocks, stored_blocks=written.stored_blocks,
                 dynamic_blocks=written.dynamic_blocks, chunks=written.chunks, spans=od.spans, span_range_reads=counts["span_range_reads"],
                 range_records=kp.range_records, stream_bytes=max([od.stream_bytes] + [pipe.store.ledger.peak for pipe in pipes]), memory_bytes=budget,
                 compressed_bytes=written.compressed_bytes, inflated_bytes=written.inflated_bytes, pos_bits=od.pos_bits,
                 passes=len(ingest_sort.digit_plan(len(opened.head.references), od.pos_bits)),
                 seconds={k: round(v, 6) for k, v in clock.times.items()})


def sort_bam(bam_path, out_path, device="cuda", range_bytes=None, chunk_bytes=None, stats=None, tables="fixed", memory_bytes=None,
             index_format="bai", pipe_bam=None, retag=None, drop_tags=None, keep_tags=None):
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
    span_range_reads (ranges read again over all spans; 0 in one piece), range_reads (the ranges and chunks read over all passes of
    the run's inputs: ``ranges`` where every input was read once, twice that where a run in one piece read its inputs a second time), range_records (the records every range of the pass
    completed), stream_bytes (the largest record buffer allocated), inputs, input_records (the records of every input), retid_inputs
    (the inputs whose records were renumbered: svx_record_retid) and the seconds per stage.  ``bam_path`` may be SAM text: then
    ``range_bytes`` is the text bytes of a chunk, and stats also has input="sam" and host_lines, the lines io/sam.py encoded.
    ``bam_path`` may be a list or tuple of such paths: their records merged into the one sorted file (see "Several inputs" at the head
    of the module); ranges and range_records run over all inputs in list order, host_lines is there when a part is SAM text, input only
    when all are; a list of one path is that path, an empty one a ValueError.  ``-`` (standard input) or a path that is no regular file
    is read once (see sort_sources._Pipe): stats also has ``pipe`` -- mode, grows, spool_bytes, text_bytes and the
    reader thread's waits; ``pipes``: the same of every such input in list order, with its name --, input="sam" as for a SAM file, and
    stream_bytes is the largest total of the pipe's record buffers.  A side effect on the calling PROCESS: when the call fails while
    ``-`` is among the inputs, descriptor 0 is pointed at the null device (textin.TextInput.close) before the error is raised -- that closes the
    pipe's read end, so that its writer ends with EPIPE and does not block; a caller that needs standard input afterwards hands the
    stream in as a path (/dev/fd/N of a duplicate) instead, whose descriptor is the call's own.  ``pipe_bam``: what becomes of a BAM
    that arrives on a pipe -- "spool" (the default): copied as it is into a file beside the output and sorted from there; "stream": a
    lone such pipe is taken in one pass, ``range_bytes`` compressed bytes a chunk (default textin.DEFAULT_PIPE_BAM_BYTES), and
    ``stats["pipe"]`` has mode "in_core" or "spooled", holds="bam" and compressed_bytes; None: ``SVX_PIPE_BAM`` of the environment.
    ``retag``: several inputs whose @RG or @PG IDs collide -- the same ID on different lines -- are merged as ``samtools merge`` does it:
    the later input's ID becomes ID-<1-based input number> in the header (sort_header.merge_headers) and the RG:Z / PG:Z values of
    that input's records are rewritten on the device (svx_record_retag_measure / svx_record_retag_write); such an input must be read
    as BAM -- SAM text that would need it is refused --, and the run reads its BAM inputs twice.  Off (the default), a colliding @RG is
    refused and a colliding @PG renamed in the header only.  None: ``SVX_SORT_RETAG=1`` of the environment turns it on.  stats:
    retag_inputs (the inputs with a table), retag_records (the records whose bytes changed); both 0, and seconds["retag"] 0.0, where
    nothing is renamed.  ``drop_tags`` / ``keep_tags``: optional fields are removed from every record as it is sorted -- a list or tuple
    of 2-character tags, or one comma-separated string; the listed fields go, or all but the listed ones (:func:`tag_filter`: the two
    exclude each other, ``CG`` always stays, a bad list is a ValueError before anything is opened).  The two files are those of the
    same inputs with the fields removed beforehand.  BAM inputs only: an input read as SAM text is refused; a lone BAM on a pipe
    keeps its spool copy under ``pipe_bam="stream"`` too; a record with malformed optional fields refuses the run.  No input is read
    twice for it, and whether the file is written in spans is decided on the unfiltered size.  Both None: ``SVX_SORT_DROP_TAGS`` /
    ``SVX_SORT_KEEP_TAGS`` of the environment.  stats: tags_mode ("drop", "keep" or None), tags_records (the records whose bytes
    changed), tags_bytes (the bytes removed); None, 0, 0 and seconds["tags"] 0.0 where the switch is off."""
    from . import kernels
    paths = input_paths(bam_path)
    tags = tag_filter(drop_tags, keep_tags)
    torch, lib, dev, clock = index.on_device("sort_bam needs the GPU (svx_record_sort, svx_bgzf_deflate)", device, STAGES)
    if tables not in TABLES:
        raise ValueError("tables: %r is none of %s" % (tables, ", ".join(TABLES)))
    if index_format not in index.FORMATS:
        raise ValueError("index_format: %r is none of %s" % (index_format, ", ".join(index.FORMATS)))
    stream_bam = textin.pipe_bam_setting(pipe_bam, "sort_bam")
    retag = os.environ.get("SVX_SORT_RETAG") == "1" if retag is None else bool(retag)
    dv = _Dev(torch, lib, kernels, dev, clock)
    chunk_blocks = max(int(chunk_bytes or DEFAULT_CHUNK_BYTES) // BLOCK, 1)
    budget = None if memory_bytes is None else max(int(memory_bytes), 1)
    ins, opened, kp, writer, counts, pipes, done = None, None, RunPass(), None, {"span_range_reads": 0}, [], False
    first_name = textin.name_of(paths[0])
    label = first_name if len(paths) == 1 else "%s (+ %d more)" % (first_name, len(paths) - 1)          # (the inputs' name in a message)
    try:
        with torch.cuda.device(dev):
            if budget is None:                                  # half of what is free: the rest is for a range, its inflate workspace, keys and chunks
                budget = max(int(torch.cuda.mem_get_info(dev)[0]) // 2, 1)
            ins = _open_all(paths, dv, _Run(out_path, chunk_blocks, budget, range_bytes, pipes, clock, stream_bam, retag, tags))
            opened = ins.merged
            opened, kp, spanned = _key_passes(dv, ins, budget, range_bytes)
            od = _order(dv, opened, kp, spanned, budget)
            pieces = _pieces_spanned if spanned else _pieces_in_core
            writer = BgzfWriter(out_path, DeviceEncode(dv, tables), clock, label)
            writer.put_header(torch.from_numpy(np.frombuffer(opened.header, np.uint8).copy()).to(dev), len(opened.header))
            for piece in pieces(dv, opened, kp, od, chunk_blocks, counts):
                writer.put(*piece)
                del piece                                       # (the chunk's buffer goes before the generator allocates the next)
            written = writer.finish()
            commit_pair(writer.tmp, out_path, _bai(opened, kp, od, written, index_format), "." + index_format)
            clock.lap("index", False)
            done = True
    except index.IndexBuildError as exc:
        raise SortWriteError("%s: %s" % (kp.reading or label, exc)) from None
    except torch.cuda.OutOfMemoryError as exc:
        raise SortWriteError("%s: the device has no room for the file's records -- %d inflated record bytes in all, %d seen so far, a budget of "
                             "%s bytes for them; a smaller one (--memory, SVX_SORT_MEMORY; sort_bam's memory_bytes) writes the file in more "
                             "spans (%s)" % (label, kp.seen if opened is None or opened.room is None else opened.room, kp.seen, budget,
                                             str(exc).split("\n")[0])) from None
    except _lib.SvxError as exc:
        raise SortWriteError("%s: %s" % (kp.reading or label, exc)) from None
    except textin.ReadError as exc:
        raise SortWriteError(str(exc)) from None
    except OSError as exc:
        raise SortWriteError("%s: writing %s failed (%s)" % (label, out_path, exc)) from None
    finally:
        for pipe in pipes:                                      # the read end first: the pipe's writer must not block on it
            pipe.input.close(failed=not done)
        if writer is not None:
            writer.discard()
        for pipe in pipes:
            pipe.discard()
    if stats is not None:
        _stats(stats, opened, kp, od, written, counts, pipes, budget, clock)
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
    ap.add_argument("--retag", action="store_true", default=os.environ.get("SVX_SORT_RETAG") == "1",
                    help="several inputs whose @RG / @PG IDs collide: rename the later input's ID to ID-<input number> and rewrite its records' "
                         "RG:Z / PG:Z tags (BAM inputs; they are read twice); without it a colliding @RG is refused (default: $SVX_SORT_RETAG=1)")
    ap.add_argument("--drop-tags", default=None, metavar="TAGS",
                    help="remove these optional fields from every record, comma-separated: fi,fp,ri,rp (BAM inputs; CG cannot be named; "
                         "default: $SVX_SORT_DROP_TAGS)")
    ap.add_argument("--keep-tags", default=None, metavar="TAGS",
                    help="remove every optional field but these (and CG): RG,NM,SA,MD; an empty list removes all (default: $SVX_SORT_KEEP_TAGS)")
    ap.add_argument("--stats-json", default=None, help="also write the statistics to this file")
    args = ap.parse_args(argv)
    try:
        tags = tag_filter(args.drop_tags, args.keep_tags)
    except ValueError as exc:
        ap.error(str(exc))
    if args.tables not in TABLES:
        ap.error("SVX_SORT_TABLES=%s: fixed or dynamic" % args.tables)
    if args.pipe_bam not in textin.PIPE_BAM + ("0",):
        ap.error("SVX_PIPE_BAM=%s: spool or stream" % args.pipe_bam)
    if os.environ.get("SVX_SORT_INDEX") not in (None, "", "bai", "csi"):
        ap.error("SVX_SORT_INDEX=%s: bai or csi" % os.environ["SVX_SORT_INDEX"])
    stats = {}
    try:
        path = sort_bam(args.bam[0] if len(args.bam) == 1 else args.bam, args.output, device=args.device, chunk_bytes=args.chunk_bytes, stats=stats, tables=args.tables,
                        memory_bytes=args.memory, pipe_bam=args.pipe_bam, retag=args.retag,
                        **({"%s_tags" % tags.mode: tags.tags} if tags is not None else {}), **(dict(index_format="csi") if args.csi else {}))
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
        if stats.get("retag_inputs"):
            print("%s: %d input(s) with renamed @RG / @PG IDs, the RG:Z / PG:Z tags of %d record(s) rewritten"
                  % (path, stats["retag_inputs"], stats["retag_records"]))
    if stats.get("tags_records"):
        print("%s: optional fields removed (--%s-tags): %d record(s) changed, %d bytes removed"
              % (path, stats["tags_mode"], stats["tags_records"], stats["tags_bytes"]))
    if stats.get("spans", 1) > 1:
        print("%s: the records exceed the budget of %d bytes (--memory): written in %d span(s), %d range(s) read again"
              % (path, stats["memory_bytes"], stats["spans"], stats["span_range_reads"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
