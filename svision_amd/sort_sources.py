"""How an input's records, keys and fields come about for svision_amd/sort.py: the four kinds of input (:class:`BamSource`,
:class:`SamSource`, :class:`PipeSource`, :class:`BamPipeSource`), how each is opened (:func:`_open`), what one input's key pass keeps
(:class:`InputPass`), and the store of a pipe's records (:class:`PipeStore`).

A source has ``key_pass(dv, opened, range_bytes, part, d_stream)``: the input's ranges -> ``part`` (the input's own :class:`InputPass`)
filled, the records' bytes kept in ``d_stream`` from byte ``part.base`` on where it is given; ``again(dv, opened, part, need) -> per
range of ``need`` (k, records completed, device bytes, the records' offsets in them [n + 1])``, the ranges of the key pass read once more
for a span; ``fill(dv, opened, part)``: the input's records written into ``part.d_stream`` behind the key passes (a run in one piece
whose ``room`` was not known before them).  ``state`` is the type of its ``part``, ``from_text``: its records come from SAM text,
``reads_once``: there is no second pass.

How an input is opened and classified, a pipe's reader owned and closed, and a chunk of text read into pinned memory and uploaded is
svision_amd/textin.py's, shared with ingest_sort.load_sample; ``is_stream`` and ``input_paths`` live there.
"""
import collections
import struct
import zlib

import numpy as np

from . import index, textin
from .sort_header import SortWriteError, sorted_header_bytes
from .sort_out import BLOCK, STREAM_SLACK, DeviceEncode, Spool, spool_copy
from .textin import is_stream

# ``remap``: None, or the int32 table of sort_header.merge_headers that takes the input's reference indices into the merged dictionary
# (a BAM input of several whose table is not the identity: svx_record_retid).
# ``pipe``: None, or the :class:`_Pipe` the input came through -- still to be read (PipeSource, BamPipeSource) or already in its spool file.
# ``text``: None, or the textin.TextInput whose chunks a SamSource or PipeSource reads.
# ``source``: the input's kind, chosen at open (the head of this module).
# ``retag``: None, or the input's table of sort_header.merge_headers(retag=True), {("RG" / "PG", old ID): new ID}: a BAM input of several
# whose @RG / @PG IDs collide with an earlier input's -- its records' RG:Z / PG:Z values are replaced (:func:`_retag`).
# ``tags``: None, or the run's :class:`TagFilter`: optional fields are removed from the input's records (:func:`_tags`; BAM inputs only).
Opened = collections.namedtuple("Opened", "path head first header room source remap pipe text retag tags", defaults=(None, None, None, None, None, None))

# Which optional fields a run removes (sort_bam's ``drop_tags`` / ``keep_tags``): ``mode`` "drop" -- the fields whose tag is in ``tags``
# go -- or "keep" -- all others go; ``CG`` stays in either mode.
TagFilter = collections.namedtuple("TagFilter", "mode tags")

# What the steps of one run share besides the device: where the output goes (a spool lies beside it), the output's chunk, the budget
# for the records' bytes, ``pipes``: every :class:`_Pipe` the run opened, for sort_bam to close and to clean up behind, and the clock.
# ``stream_bam``: a lone BAM on a pipe is taken in one pass (``pipe_bam="stream"``), not copied into a file first.
# ``retag``: colliding @RG / @PG IDs of several inputs are renamed and the records follow (sort_bam's ``retag``).
# ``tags``: None, or the :class:`TagFilter` of the run.
_Run = collections.namedtuple("_Run", "out_path chunk_blocks budget range_bytes pipes clock stream_bam retag tags", defaults=(False, False, None))


def inflated_size(path):
    """The sum of the members' ISIZE fields: the file's inflated bytes, from its headers and footers alone."""
    try:
        return sum(isize for _at, _bsize, _xlen, isize in index.bgzf_members(path))
    except index.IndexBuildError as exc:
        raise SortWriteError(str(exc)) from None


# ---- what one input's key pass keeps ----
class InputPass:
    """What the key pass over ONE input leaves, filled as it goes: per range ``range_records`` and ``places``; ``seen``: the inflated
    record bytes so far; what the join takes of the ranges (``host``, ``d_keys``, ``lens``: per range the host fields, the device keys,
    the records' lengths; emptied behind it); ``base``: the stream offset of its first record; and behind the join its ``n`` records'
    slices of the run's ``off_in`` / ``d_off_in`` -- offsets in the one stream -- and, while it is filled, the run's ``d_stream``.
    ``range_reads``: the ranges (chunks) of the input read so far, over all its passes -- ``len(range_records)`` where it was read once."""

    def __init__(self, base=0):
        self.range_records, self.places, self.seen, self.n, self.base, self.range_reads = [], [], 0, 0, base, 0
        self.host, self.d_keys, self.lens = [], [], []
        self.off_in = self.d_off_in = self.d_stream = None

    def drop_keys(self):
        """What the join takes goes: it has been joined, or the records went to a spool whose own key pass computes it again."""
        self.host, self.d_keys, self.lens = [], [], []


class BamPass(InputPass):
    """A BAM's: ``d_map`` besides, the input's ``remap`` on the device once :func:`_retid` has needed it; ``d_retag``: its ``retag``
    table likewise (:func:`_retag`), ``retag_records``: the records the key pass rewrote; ``read``: the record bytes as the file
    holds them, which ``seen`` is not where records were rewritten; ``d_tags``: the bitmap of the run's :class:`TagFilter`
    (:func:`_tags`), ``tags_records`` / ``tags_bytes``: the records the key pass shortened and the bytes it removed."""

    def __init__(self, base=0):
        InputPass.__init__(self, base)
        self.d_map = self.d_retag = self.d_tags = None
        self.retag_records = self.read = self.tags_records = self.tags_bytes = 0


class SamPass(InputPass):
    """SAM text's: ``host_lens`` per chunk the lines' lengths as svx_sam_encode takes them (negative: the host's line),
    ``host_records`` {record number: the bytes io.sam encoded}, ``tid_of`` / ``sam_table``: the host's and the device's reference
    names, ``reader``: the textin.ChunkReader of the text, with the pinned memory a chunk is read into."""

    def __init__(self, base=0):
        InputPass.__init__(self, base)
        self.host_lens, self.host_records, self.tid_of, self.sam_table, self.reader = [], {}, None, None, None


def _rec_base(kp):
    """The number of the first record of every range of the key pass, and behind the last [ranges + 1]."""
    return np.concatenate([[0], np.cumsum(np.asarray(kp.range_records, np.int64))])


# A range's (a chunk's) records as the key pass measured them: the number of the first one in its input, the records' lengths, (SAM) the
# lengths as svx_sam_encode takes them, tid pos flag span on the host -- in the merged numbering --, the keys on the device, and (BAM)
# ``at``: the byte of the first record in the range's inflated stream, where the records lie end to end.
Measured = collections.namedtuple("Measured", "first length kernel_len tid pos flag span d_tid d_pos at", defaults=(None,))


def _keep_measured(part, place, m, keys=True):
    """A measured range or chunk into the input's pass -- the only place that appends to it; ``keys`` unset (its records go to a
    spool): without what the join takes of it."""
    part.range_records.append(m.length.size)
    part.places.append(place)
    if m.kernel_len is not None:
        part.host_lens.append(m.kernel_len)
    if keys and m.length.size:
        part.host.append((m.tid, m.pos, m.flag, m.span))
        part.lens.append(m.length)
        part.d_keys.append((m.d_tid, m.d_pos))
    part.seen += int(m.length.sum())


# ---- a BAM's ranges ----
def _retid(dv, opened, part, d_bytes, d_off, d_tid_key):
    """The records at ``d_off`` in ``d_bytes`` of an input whose reference indices are not the merged dictionary's: refID and next_refID
    -- and the sort's key -- through the input's table (svx_record_retid)."""
    torch = dv.torch
    if part.d_map is None:
        part.d_map = torch.from_numpy(np.ascontiguousarray(opened.remap, np.int32)).to(dv.dev)
    d_status = torch.zeros(1, dtype=torch.int32, device=dv.dev)
    dv.kernels.record_retid(d_bytes, d_off, part.d_map, d_tid_key, d_status)
    bad = int(d_status.item())
    dv.clock.lap("retid")
    if bad:
        raise SortWriteError("%s: a record's reference index is outside its file's dictionary (%d references)" % (opened.path, len(opened.remap)))


def _retag(dv, opened, part, d_bytes, d_off, count=False):
    """The records at ``d_off`` [n + 1] in ``d_bytes`` of an input whose @RG / @PG IDs were renamed in the merged header -> (a new
    buffer, the records' offsets in it [n + 1]): svx_record_retag_measure, an exclusive sum, svx_record_retag_write -- the first RG:Z
    and PG:Z value that the input's table holds replaced, block_size with it; the status is read once.  The buffer has the 4
    readable bytes behind its records that the gather and the scatter want.  ``count``: the key pass, which counts the records
    that changed."""
    torch, kernels = dv.torch, dv.kernels
    if part.d_retag is None:
        part.d_retag = kernels.retag_table(opened.retag, dv.dev)
    n = int(d_off.shape[0]) - 1
    d_status = torch.zeros(1, dtype=torch.int32, device=dv.dev)
    d_len = kernels.record_retag_measure(d_bytes, d_off, part.d_retag, d_status)
    d_new_off = torch.zeros(n + 1, dtype=torch.int64, device=dv.dev)
    torch.cumsum(d_len, 0, out=d_new_off[1:])
    total = int(d_new_off[n].item())
    d_out = torch.empty(total + 4, dtype=torch.uint8, device=dv.dev)
    d_out[total:] = 0
    kernels.record_retag_write(d_bytes, d_off, part.d_retag, d_new_off, d_out, d_status)
    if count:
        part.retag_records += int((d_len != d_off[1:] - d_off[:-1]).sum().item())
    bad = int(d_status.item())
    dv.clock.lap("retag")
    if bad:
        raise SortWriteError("%s: a record's optional fields are malformed -- its RG:Z / PG:Z tags cannot be rewritten" % opened.path)
    return d_out, d_new_off


def _tags(dv, opened, part, d_bytes, d_off, count=False):
    """The records at ``d_off`` [n + 1] in ``d_bytes`` of an input under the run's :class:`TagFilter` -> (a new buffer, the records'
    offsets in it [n + 1]): svx_record_tags_measure, an exclusive sum, svx_record_tags_write -- every optional field that the filter
    removes gone, block_size with it; the status is read once.  The buffer has the 4 readable bytes behind its records that the
    gather and the scatter want.  ``count``: the key pass, which counts the records that changed and the bytes that went."""
    torch, kernels = dv.torch, dv.kernels
    if part.d_tags is None:
        part.d_tags = kernels.tags_table(opened.tags.tags, opened.tags.mode == "keep", dv.dev)
    n = int(d_off.shape[0]) - 1
    d_status = torch.zeros(1, dtype=torch.int32, device=dv.dev)
    d_len = kernels.record_tags_measure(d_bytes, d_off, part.d_tags, d_status)
    d_new_off = torch.zeros(n + 1, dtype=torch.int64, device=dv.dev)
    torch.cumsum(d_len, 0, out=d_new_off[1:])
    total = int(d_new_off[n].item())
    d_out = torch.empty(total + 4, dtype=torch.uint8, device=dv.dev)
    d_out[total:] = 0
    kernels.record_tags_write(d_bytes, d_off, part.d_tags, d_new_off, d_out, d_status)
    if count:
        part.tags_records += int((d_len != d_off[1:] - d_off[:-1]).sum().item())
        part.tags_bytes += int((d_off[n] - d_off[0]).item()) - total
    bad = int(d_status.item())
    dv.clock.lap("tags")
    if bad:
        raise SortWriteError("%s: a record's optional fields are malformed -- they cannot be filtered (--drop-tags / --keep-tags)" % opened.path)
    return d_out, d_new_off


def _bam_measured(dv, opened, part, rng, room=None):
    """A walked range of a BAM -- a file's or a streamed pipe's -> Measured: svx_cigar_scan for the reference spans
    (index._index_fields), the records' lengths from their offsets up to the chain's exit, and, for an input with a ``remap``, the
    range's records and keys translated where they lie (:func:`_retid`), the host's tid too.  ``room``: the record bytes the file's ISIZE
    fields add up to; more than that -- of the bytes as they were read -- is refused before anything is rewritten.  An input with a
    ``retag`` table: the range's records and offsets are then replaced by the rewritten ones (:func:`_retag`), so lengths, ``seen``
    and everything behind see those.  An input under a :class:`TagFilter`: likewise, behind the retag (:func:`_tags`)."""
    first = sum(part.range_records)
    if not rng.n_rec:
        return Measured(first, np.empty(0, np.int64), None, None, None, None, None, None, None, 0)
    tid, pos, flag, span, rec_off = index._index_fields(dv.lib, dv.torch, dv.kernels, dv.dev, rng, dv.clock)
    at, last = int(rec_off[0]), int(rng.exit_off)
    if room is not None and part.read + last - at > room:
        raise SortWriteError("%s: more record bytes than its BGZF blocks' ISIZE fields add up to (%d)" % (opened.path, room))
    part.read += last - at
    if opened.remap is not None:
        _retid(dv, opened, part, rng.d_raw, rng.d_rec_off, rng.d_tid)
        tid = np.where(tid >= 0, opened.remap[np.maximum(tid, 0)], tid).astype(np.int32)
    if opened.retag or opened.tags:
        d_new_off = dv.torch.cat([rng.d_rec_off, dv.torch.tensor([last], dtype=dv.torch.int64, device=dv.dev)])
        if opened.retag:
            rng.d_raw, d_new_off = _retag(dv, opened, part, rng.d_raw, d_new_off, count=True)
        if opened.tags:
            rng.d_raw, d_new_off = _tags(dv, opened, part, rng.d_raw, d_new_off, count=True)
        rng.d_rec_off = d_new_off[:-1]
        return Measured(first, np.diff(d_new_off.cpu().numpy()), None, tid, pos, flag, span, rng.d_tid, rng.d_pos, 0)
    length = np.diff(np.append(rec_off, np.uint64(last)).astype(np.int64))
    return Measured(first, length, None, tid, pos, flag, span, rng.d_tid, rng.d_pos, at)


def _release(rng):
    """A range's device arrays go -- all but the keys, which the pass may have kept -- so that, once the caller has dropped the range
    itself, the generator makes the next one in their room."""
    rng.d_raw = rng.d_starts = rng.d_base = rng.d_cigar = rng.d_cig_off = rng.d_names = rng.d_name_off = rng.d_rec_off = None


class BamSource:
    """A BAM file.

      pass      the whole file in ranges, the loop of the index build (index.record_ranges): read, inflate, CRC, svx_bam_find_starts, the
                walk, svx_cigar_scan for the reference spans (index._index_fields).  Kept per range: tid and pos on the device; tid, pos,
                flag, span and the records' byte offsets on the host; and the BYTES of the records that complete in the range, the slice
                [first record, exit_off) of the range's inflated stream.  CIGAR words, names and the rest of the range are dropped
      key pass  (a run in spans) the pass above keeping no record byte: keys on the device, fields and the records' lengths on the host,
                and per range its place in the file and the number of records it completed
      span pass per span, the ranges that own a record of it (sort.span_ranges) and no others are read again: read, inflate, CRC,
                svx_bam_find_starts, the walk's counts and svx_bam_walk_offsets -- no field, CIGAR word or name is extracted, no CIGAR
                scanned -- and ONE svx_record_scatter_segments a range puts its records of the span at their output offsets in the
                span's buffer.  A nearly sorted input costs about one extra read of the file, a shuffled one a read a span.  A range that
                completes another number of records than in the key pass, or a record of another length, means the file changed:
                SortWriteError

    One of several inputs is walked against ITS OWN dictionary (svx_bam_find_starts validates against it).  Where its table is not the
    identity, svx_record_retid -- a lane a record -- rewrites refID and next_refID of the range's records where they lie, and the
    sort's key with them, before the slice is kept; the host's tid goes through the table in NumPy.  Identical dictionaries, or one that
    opens the merged one: no launch.  A reference index outside the file's dictionary: SortWriteError.

    One of several inputs whose @RG / @PG IDs collide with an earlier input's, under ``retag``: the merged header renamed them, and the
    records' RG:Z / PG:Z values follow (:func:`_retag`: svx_record_retag_measure, an exclusive sum, svx_record_retag_write -- a wave a
    record).  A rewritten record has another length, so the input's record bytes are known only behind its key pass: the run keeps no
    byte in the key passes and reads its BAM inputs a second time (``fill``) or in spans (``again``), where the same rewriting gives the
    same lengths; the ISIZE check stays on the bytes as read.  An input with no table: no launch, no allocation.

    Under the run's :class:`TagFilter` (``drop_tags`` / ``keep_tags``) every range's records lose the optional fields it removes
    (:func:`_tags`: svx_record_tags_measure, an exclusive sum, svx_record_tags_write -- a wave a record), behind the renumbering and
    the retag.  Records only get shorter, so the ISIZE sum stays an upper bound of the input's record bytes: ``room`` stays that sum,
    the stream is allocated once and the shortened records are kept end to end as the key passes go -- no second read; whether the
    run is written in spans is decided on the unfiltered size.  In spans ``again`` filters the range's records again: the same lengths."""
    name, state, from_text, reads_once = "bam", BamPass, False, False

    def key_pass(self, dv, opened, range_bytes, part, d_stream):
        """key pass of a BAM: every range of the file (index.record_ranges) -> ``part`` filled.  ``d_stream``: the record stream, allocated
        once by the ISIZE sum -- every range's slice goes straight to its place in it, from byte ``part.base`` on --, or None: no byte is
        kept."""
        for rng in index.record_ranges(opened.path, opened.head, dv.dev, dv.clock, range_bytes, first=opened.first):
            part.range_reads += 1
            m = _bam_measured(dv, opened, part, rng, opened.room)
            if d_stream is not None and m.length.size:
                at, need = part.base + part.seen, int(m.length.sum())
                d_stream[at:at + need].copy_(rng.d_raw[m.at:m.at + need])       # the records that complete in the range: contiguous there
            _keep_measured(part, rng.place, m)
            _release(rng)
            del rng, m
            dv.clock.lap("keep")

    def again(self, dv, opened, part, need):
        """The ranges ``need`` of a BAM read again: read, inflate, CRC, find_starts, the walk's counts and offsets; nothing is extracted.
        An input with a ``remap``: the range's records translated where they lie before they are handed on (:func:`_retid`); with a
        ``retag`` table: the rewritten records and their offsets are handed on (:func:`_retag`); under a :class:`TagFilter`: the
        filtered ones (:func:`_tags`)."""
        for k, rng in zip(need, index.record_ranges(opened.path, opened.head, dv.dev, dv.clock, places=[part.places[k] for k in need], extract=False,
                                                    first=opened.first)):
            part.range_reads += 1
            if rng.n_rec != part.range_records[k]:
                yield k, rng.n_rec, None, None                  # (the caller refuses it; no offsets are taken of a range that changed)
                return
            d_src_off = index.walk_offsets(dv.lib, dv.torch, dv.kernels, dv.dev, rng, closed=True)
            dv.clock.lap("walk")
            if opened.remap is not None:
                _retid(dv, opened, part, rng.d_raw, d_src_off[:rng.n_rec], None)
            if opened.retag:
                rng.d_raw, d_src_off = _retag(dv, opened, part, rng.d_raw, d_src_off)
            if opened.tags:
                rng.d_raw, d_src_off = _tags(dv, opened, part, rng.d_raw, d_src_off)
            yield k, rng.n_rec, rng.d_raw, d_src_off
            _release(rng)
            del rng, d_src_off

    def fill(self, dv, opened, part):
        """in one piece, a BAM beside SAM text (``room`` was not known before the key passes): the ranges that completed a record READ A
        SECOND TIME -- the path of the spans without the scatter --, each range's records -- contiguous in the range and in the stream
        -- one copy.  That second read is the price of a mixed run (profiles/sort_merge.txt); an all-BAM run does not pay it."""
        need = np.flatnonzero(np.asarray(part.range_records, np.int64))
        rec_base = _rec_base(part)
        for k, n_rec, d_raw, d_src_off in self.again(dv, opened, part, need) if need.size else ():
            ends = [int(v) for v in d_src_off[[0, n_rec]].cpu()] if n_rec == part.range_records[k] else None
            at, end = int(part.off_in[rec_base[k]]), int(part.off_in[rec_base[k + 1]])
            if ends is None or ends[1] - ends[0] != end - at:
                raise SortWriteError("%s changed while it was sorted: the range at file offset %d does not complete the records it did in the "
                                     "first pass" % (opened.path, part.places[k][0]))
            part.d_stream[at:end].copy_(d_raw[ends[0]:ends[1]])
            dv.clock.lap("keep")
            del d_raw, d_src_off


# ---- a SAM's chunks of text ----
def _sam_measured(dv, opened, part, chunk, d_text, d_line_off, n_lines):
    """A chunk's lines measured (svx_sam_measure) and read back -> Measured(the number of the chunk's first record, the records' lengths
    with the host's lines patched in, the lengths as svx_sam_encode takes them, tid, pos, flag, span on the host, the keys on the device).
    An error code raises with the line's number -- ``chunk.line_no`` lines lie in front of the chunk --; a line the kernels leave to the
    host is encoded by io.sam.encode_line and kept in ``part.host_records`` by record number.  A pass's first call sets ``part``'s names."""
    from .io import sam
    if part.sam_table is None:
        part.tid_of, part.sam_table = sam.tid_table(opened.head.references), dv.kernels.sam_ref_table(opened.head.references, dv.dev)
    torch, kernels, dev, clock = dv.torch, dv.kernels, dv.dev, dv.clock
    d_len, d_tid, d_pos, d_flag, d_span = kernels.sam_measure(d_text, chunk.n, d_line_off, n_lines, part.sam_table)
    clock.lap("measure")
    length, tid, pos, flag, span = (t.cpu().numpy() for t in (d_len, d_tid, d_pos, d_flag, d_span))
    line_off = d_line_off[:n_lines + 1].cpu().numpy()
    clock.lap("read_back")
    bad = np.flatnonzero(length < kernels.SAM_HOST)
    if bad.size:
        i = int(bad[0])
        raise SortWriteError("%s: %s" % (opened.path, textin.line_refusal(textin.line_bytes(chunk.data, line_off, i), part.tid_of, chunk.line_no + i + 1,
                                                                      "svx_sam_measure", int(length[i]))))
    kernel_len, first = length.copy(), sum(part.range_records)
    left = np.flatnonzero(length == kernels.SAM_HOST)
    for i in left:
        line = textin.line_bytes(chunk.data, line_off, i)
        try:
            rec = sam.encode_line(line, part.tid_of)
            tid[i], pos[i], flag[i], span[i] = sam.fields_of(line, part.tid_of)
        except sam.SamError as exc:
            raise SortWriteError("%s: %s" % (opened.path, exc.at(chunk.line_no + int(i) + 1))) from None
        length[i] = len(rec)
        part.host_records[first + int(i)] = rec
    if left.size:
        d_tid, d_pos = torch.from_numpy(tid).to(dev), torch.from_numpy(pos).to(dev)
    clock.lap("host_lines", False)
    return Measured(first, length.astype(np.int64), kernel_len, tid, pos, flag.astype(np.uint16), span, d_tid, d_pos)


def _place_host_records(torch, take, kernel_len, first, off, d_out):
    """A chunk's records that the host encoded (``kernel_len`` < 0), ``take(first + i)`` each, copied to ``off[i]`` in ``d_out`` -> how many."""
    left = np.flatnonzero(kernel_len < 0)
    for i in left:
        rec = take(first + int(i))
        d_out[int(off[i]):int(off[i]) + len(rec)].copy_(torch.frombuffer(bytearray(rec), dtype=torch.uint8))
    return left.size


def _sam_encode_chunk(dv, opened, part, k, first, base, d_out, d_status):
    """Chunk k of the key pass read again and its records written: svx_sam_lines -> svx_sam_encode to ``d_out``, record r of the stream
    at byte off_in[r] - base; the host's encodings copied to their offsets.  ``first``: the number of the chunk's first record.
    -> the lines the chunk has now (another number than in the key pass: nothing is written)."""
    torch, kernels = dv.torch, dv.kernels
    try:
        chunk = part.reader.at(opened.text, part.places[k])
    except textin.ReadError as exc:
        raise SortWriteError("%s changed while it was sorted: %s" % (exc.path, exc.what)) from None
    d_text, d_line_off, n_lines = textin.upload_lines(torch, kernels, dv.dev, dv.clock, chunk)
    part.range_reads += 1
    if n_lines != part.range_records[k]:
        return n_lines
    d_len = torch.from_numpy(part.host_lens[k]).to(dv.dev)
    kernels.sam_encode(d_text, chunk.n, d_line_off, n_lines, part.sam_table, d_len, part.d_off_in[first:first + n_lines], base, d_out, d_status)
    dv.clock.lap("encode")
    _place_host_records(torch, part.host_records.__getitem__, part.host_lens[k], first, part.off_in[first:first + n_lines] - base, d_out)
    dv.clock.lap("host_lines")
    return n_lines


class SamSource:
    """SAM text.  An aligner's output that was never converted (minimap2, winnowmap, ngmlr, pbmm2 without --sort) is taken as it is: a file
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
      in spans  the places of sort.span_ranges are chunks of text: each is encoded into a chunk-local buffer and goes through
                svx_record_scatter_segments like a BAM's range.  A chunk with another number of lines, or a line whose record has another
                length than in the key pass, means the file changed: SortWriteError
    A regular file of compressed SAM (gzip, BGZF) is not taken: the text of a file is read twice, and there is no device decoder for it.
    Among several inputs SAM text is measured and encoded against the MERGED names, so it needs no table, and a part without any header
    is usable beside one that has it."""
    name, state, from_text, reads_once = "sam", SamPass, True, False

    def key_pass(self, dv, opened, range_bytes, part, d_stream=None):
        """key pass of SAM text: one pass over the chunks (textin.ChunkReader.chunks: ``range_bytes`` of text, cut at line ends): svx_sam_lines,
        svx_sam_measure, the lengths and fields read back.  An error code raises with the file's line number; a line the kernels leave to the
        host (SVX_SAM_HOST) is encoded by io.sam at once -- its bytes kept in ``part.host_records`` by record number, its length, key and
        fields patched in.  No byte is kept: ``room`` is exact behind the pass, and a run in one piece then reads the text once more
        (:meth:`fill`)."""
        part.reader = textin.ChunkReader(dv.torch, dv.lib, dv.clock)
        for chunk in part.reader.chunks(opened.text, range_bytes):
            part.range_reads += 1
            d_text, d_line_off, n_lines = textin.upload_lines(dv.torch, dv.kernels, dv.dev, dv.clock, chunk)
            _keep_measured(part, chunk.place, _sam_measured(dv, opened, part, chunk, d_text, d_line_off, n_lines))
            del d_text, d_line_off
            dv.clock.lap("keep")

    def again(self, dv, opened, part, need):
        """The chunks ``need`` of SAM text read again for a span: each encoded into a chunk-local buffer (+ the 4 readable bytes the
        scatter's aligned loads want) whose record offsets are the key pass's."""
        torch, dev = dv.torch, dv.dev
        rec_base = _rec_base(part)
        for k in need:
            first, n_rec = int(rec_base[k]), int(part.range_records[k])
            base = int(part.off_in[first])
            d_local = torch.zeros(int(part.off_in[first + n_rec]) - base + 4, dtype=torch.uint8, device=dev)
            d_status = torch.zeros(1, dtype=torch.int32, device=dev)
            d_src_off = part.d_off_in[first:first + n_rec + 1] - base
            n_lines = _sam_encode_chunk(dv, opened, part, k, first, base, d_local, d_status)
            if n_lines == n_rec and int(d_status.item()):
                raise SortWriteError("%s changed while it was sorted: a line's record is not of the length the first pass saw" % opened.path)
            yield k, n_lines, d_local, d_src_off
            del d_local, d_src_off

    def fill(self, dv, opened, part):
        """in one piece, SAM text: the second read of the text -- in the page cache for a file that fits the device --, every chunk encoded
        straight into the resident stream (``part.d_stream``) at its records' offsets."""
        d_status = dv.torch.zeros(1, dtype=dv.torch.int32, device=dv.dev)
        for k, first in enumerate(_rec_base(part)[:-1]):
            n_lines = _sam_encode_chunk(dv, opened, part, k, int(first), 0, part.d_stream, d_status)
            if n_lines != part.range_records[k]:
                raise SortWriteError("%s changed while it was sorted: %d lines complete in the chunk at file offset %d, %d did in the first pass"
                                     % (opened.path, n_lines, part.places[k][0], part.range_records[k]))
        if int(d_status.item()):
            raise SortWriteError("%s changed while it was sorted: a line's record is not of the length the first pass saw" % opened.path)


# ---- a pipe: an input that is seen once ----
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


class PipeStore:
    """The records of a pipe as they arrive, a chunk's (a range's) at a time: kept on the device while :func:`keeps_in_core` says so,
    in the spool file from the first refusal on.  ``mode`` ("in_core", "spooled"; "bam_spooled": a BAM that was copied as it is, which
    never comes here) says which to the caller, ``ledger`` what lay on the device.

      the stream grows  by a segment a chunk: nothing is copied while the input arrives and nothing is allocated ahead, so what lies on the
                device is the record bytes seen so far -- a small pipe takes a small share of the card.  At the end of the input the
                segments are joined into the one resident stream (:meth:`fill`; each goes when it is copied): then, and only then, both
                copies exist.  :func:`keeps_in_core` keeps a chunk while that join still fits ``budget``; so (a) the source's record
                buffers never exceed the budget, (b) never twice the record bytes seen plus one chunk's records -- and a pipe stays in core
                up to HALF the budget, where a file does up to all of it.  ``stats["stream_bytes"]``: the largest total, the join's
      the spool beyond it, the source switches to :class:`Spool` and does not fail: an unsorted BAM beside the output, ``out_path +
                ".spool.<pid>.bam"``, under the stream's header, written through :class:`BgzfWriter` with :class:`DeviceEncode` in the fixed
                code -- the records kept so far first, joined into one buffer, which the rule has left room for, then every later
                chunk's as they are encoded, in arrival order (a chunk's buffer is in transit, like a span pass's chunk-local one, and
                not kept).  At the end of the input the pass's own results are dropped and the input BECOMES that file: the BAM road,
                key pass, spans, ``again``.  One extra write and two reads of BAM-sized data, paid only by a pipe that does not fit

    Per chunk of ``need`` record bytes: :meth:`admit` decides, :meth:`buffer` hands out exactly ``need`` bytes (spooling: + STREAM_SLACK,
    zeroed) for the caller to write the records into, :meth:`keep` takes the buffer back -- a segment, or put to the spool at once.
    Like :class:`BgzfWriter` it is handed what touches the device (:meth:`on`): ``header() -> the spool's header bytes``, ``alloc(n_bytes)``,
    ``copy(destination, segment)``, the spool's ``encode`` and ``as_buffer``; torch in the key passes, NumPy in tests/test_sort_pipe_cpu.py."""

    def __init__(self, out_path, budget, step, clock, name=None, number=0):
        self.out_path, self.budget, self.step, self.clock, self.name, self.number = out_path, budget, step, clock, name, number
        self.mode, self.ledger, self.segments, self.kept = "in_core", StreamLedger(), [], 0
        self.spool, self.spool_file, self.spool_bytes = None, None, 0

    def on(self, header, alloc, copy, encode, as_buffer):
        self.header, self.alloc, self.copy, self.encode, self.as_buffer = header, alloc, copy, encode, as_buffer
        return self

    def to_spool(self):
        """The budget does not hold the next chunk (or the pipe is one of several inputs): the spool file is opened, and the records
        kept so far go in first."""
        self.mode = "spooled"
        self.spool = Spool(self.out_path, self.header(), self.encode, self.clock, self.as_buffer, self.name, self.number)
        if self.segments:
            kept = self.kept
            buf = self.alloc(kept + STREAM_SLACK)
            self.ledger.add(kept + STREAM_SLACK)
            buf[kept:] = 0
            self.join(buf)
            self.spool.put(buf, kept, self.step)
            self.ledger.drop(kept + STREAM_SLACK)
            del buf

    def admit(self, need):
        """A chunk that brings ``need`` record bytes -> True where it is the first the rule refuses: the spool was opened."""
        if self.spool is not None or not need or keeps_in_core(self.kept, need, self.budget):
            return False
        self.to_spool()
        return True

    def buffer(self, need):
        buf = self.alloc(need + (STREAM_SLACK if self.spool is not None else 0))
        buf[need:] = 0
        return buf

    def keep(self, buf, need):
        if self.spool is not None:
            self.spool.put(buf, need, self.step)
        elif need:
            self.segments.append(buf)
            self.kept += need
            self.ledger.add(need)

    def join(self, out, at=0):
        """The segments end to end into ``out`` from byte ``at`` on; each goes when it is copied."""
        for k, seg in enumerate(self.segments):
            n = len(seg)
            self.copy(out[at:at + n], seg)
            at += n
            self.segments[k] = None
            self.ledger.drop(n)
            del seg
        self.segments, self.kept = [], 0
        self.clock.lap("keep")
        return at

    def fill(self, out, at):
        """in one piece: the segments joined into the resident stream ``out`` -- both copies exist while they are."""
        self.ledger.add(len(out))
        self.join(out, at)

    def finish(self):
        """The end of the input: a spool is closed and put in place."""
        if self.spool is not None:
            self.spool_file, self.spool_bytes = self.spool.finish(), self.spool.bytes

    def discard(self):
        self.segments = []
        if self.spool is not None:
            self.spool.discard()
        index.discard(self.spool_file)


class _Pipe:
    """An input that is read once -- standard input, a FIFO, /dev/fd/N -- as the sort keeps it: the textin.TextInput that owns its
    reader, its name in messages (``<stdin>`` for ``-``), its :class:`PipeStore` (the mode, the ledger of its record buffers on the
    device, the spool beyond the budget) and what the statistics report.  :meth:`discard` removes the spool; closing is the input's
    (textin.TextInput.close).

    A pipe.  ``minimap2 -a ref.fa reads.fq | python -m svision_amd.sort - -o sorted.bam``: ``-`` is standard input (``<stdin>`` in messages),
    and any path that os.stat says is no regular file -- a FIFO, /dev/fd/N, ``<(winnowmap -a ...)`` -- takes the same road, decided
    before a byte is read.  The text is seen ONCE, and the two files are those of the same bytes read from a regular file.
    On any failure the read end is closed BEFORE the error is raised -- standard input is pointed at the null device --, so that the
    pipe's writer ends with EPIPE / SIGPIPE and does not block on a full pipe; no output, no temporary and no spool is left.  An early
    end of the writer is no error by itself: what arrived is the input, and a cut last line fails by the parser's rules with its number.
    ``stats["pipe"]``: mode ("in_core", "spooled", "bam_spooled"), holds ("sam", "bam": what the pipe held), grows (segments + the join),
    spool_bytes, text_bytes (the bytes read: of a BAM its compressed bytes, ``compressed_bytes`` too), and the seconds the reader's
    thread waited for the pipe and for a free buffer."""

    def __init__(self, inp, run):
        self.input, self.name, self.run, self.number = inp, inp.name, run, len(run.pipes)
        self.store = PipeStore(run.out_path, run.budget, run.chunk_blocks * BLOCK, run.clock, self.name, self.number)
        self.host_lines = 0
        self.holds, self.bam_header = "sam", None               # what the pipe held; a streamed BAM: the bytes in front of its first record

    def on_device(self, dv, header):
        """-> the store, handed the device: torch buffers, the fixed-code encoder; ``header()``: the spool's header bytes."""
        torch = dv.torch
        return self.store.on(header, lambda n_bytes: torch.empty(n_bytes, dtype=torch.uint8, device=dv.dev), lambda d_out, d_seg: d_out.copy_(d_seg),
                             DeviceEncode(dv, "fixed"), lambda b: torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(dv.dev))

    def discard(self):
        self.store.discard()

    def stats(self):
        reader, store = self.input.reader, self.store
        return dict(mode=store.mode, holds=self.holds, grows=store.ledger.grows, spool_bytes=store.spool_bytes, text_bytes=reader.text_bytes,
                    reader_wait_pipe_s=round(reader.wait_pipe, 6), reader_wait_buffer_s=round(reader.wait_buffer, 6),
                    **(dict(compressed_bytes=reader.text_bytes) if self.holds == "bam" else {}))


class PipeSource(SamSource):
    """SAM text on a pipe."""
    name, reads_once = "pipe", True

    def key_pass(self, dv, opened, range_bytes, part, d_stream=None, spool_header=None):
        """key pass of a pipe, the ONLY pass over its text: the reader's thread drains the pipe into two pinned buffers, chunks of
        ``range_bytes`` cut by the rule of io.sam.chunk_places, while the device works on the chunk before; per chunk upload,
        svx_sam_lines, svx_sam_measure, the read-back and the host's lines as :meth:`SamSource.key_pass` has them -- with the stream's
        line numbers -- and AT ONCE svx_sam_encode: the chunk's records into a SEGMENT of exactly their bytes, their offsets the exclusive
        sum of the lengths behind the bytes kept so far; the host's encodings copied to theirs.  Keys, fields, lengths,
        ``range_records`` and ``host_lens`` are kept as for a file; :meth:`fill` joins the segments.  A chunk that the
        :class:`PipeStore` refuses (``spool_header`` given: the first) opens the spool: from then on every chunk's records are appended
        to it in arrival order and nothing is kept; ``opened.pipe.store.mode`` says so to the caller."""
        from .io import sam
        torch, kernels, dev, clock, pipe = dv.torch, dv.kernels, dv.dev, dv.clock, opened.pipe
        store = pipe.on_device(dv, lambda: sam.bam_header_bytes(opened.head) if spool_header is None else spool_header)
        part.reader = textin.ChunkReader(torch, dv.lib, clock)
        if spool_header is not None:
            store.to_spool()
        d_status = torch.zeros(1, dtype=torch.int32, device=dev)
        for chunk in part.reader.chunks(opened.text, range_bytes):
            part.range_reads += 1
            d_text, d_line_off, n_lines = textin.upload_lines(torch, kernels, dev, clock, chunk)
            m = _sam_measured(dv, opened, part, chunk, d_text, d_line_off, n_lines)
            need = int(m.length.sum())
            if store.admit(need):
                part.drop_keys()
            off = np.cumsum(m.length) - m.length
            d_seg = store.buffer(need)
            if n_lines:
                kernels.sam_encode(d_text, chunk.n, d_line_off, n_lines, part.sam_table, torch.from_numpy(m.kernel_len).to(dev),
                                   torch.from_numpy(off + part.seen).to(dev), part.seen, d_seg, d_status)
            clock.lap("encode")
            pipe.host_lines += _place_host_records(torch, part.host_records.pop, m.kernel_len, m.first, off, d_seg)
            clock.lap("host_lines")
            if int(d_status.item()):
                raise SortWriteError("%s: a line's record is not of the length svx_sam_measure gave it" % opened.path)
            store.keep(d_seg, need)
            _keep_measured(part, chunk.place, m, keys=store.spool is None)
            del d_text, d_line_off, d_seg
            clock.lap("keep")
        opened.text.close()
        store.finish()

    def again(self, dv, opened, part, need):
        raise SortWriteError("%s: a pipe cannot be read again" % opened.path)  # (not reached: a pipe beyond the budget is spooled)

    def fill(self, dv, opened, part):
        """in one piece, a pipe: its segments joined into the resident stream (``part.d_stream``)."""
        opened.pipe.store.fill(part.d_stream, int(part.off_in[0]) if part.n else part.base)


class BamPipeSource(BamSource):
    """A BAM on a pipe, streamed.  ``pipe_bam="stream"`` (``--pipe-bam stream``, ``SVX_PIPE_BAM=stream``; off by default: measured, it wins in
    core and loses once it spools, profiles/pipe_bam.txt and DESIGN section 9) takes a LONE such pipe in one pass: the header
    through zlib from the stream (io.sam.StreamReader.bam_header), the BGZF members in chunks of ``range_bytes`` compressed
    bytes (textin.member_chunks: the reader's thread, pinned buffers), and per range the BAM key pass over index.stream_ranges,
    which carries a cut record's compressed blocks into the next range where a file's pass seeks back.  A range's records
    ``d_raw[first:exit_off]`` are a segment of exactly their size; :func:`keeps_in_core`, the spool beyond the budget (the
    kept records first, then every range's), the join and the statistics are the text pipe's.  In core no spool file exists
    at any moment.  Among several inputs a BAM pipe keeps the copy as it is under either setting: it would be spooled from its
    first byte anyway, and the copy is the cheapest form of that."""
    name, reads_once, again, fill = "bam_pipe", True, PipeSource.again, PipeSource.fill

    def key_pass(self, dv, opened, range_bytes, part, d_stream=None):
        """key pass of a BAM on a pipe, the ONLY pass over it: :meth:`BamSource.key_pass`'s body per range of index.stream_ranges
        (:func:`_bam_measured`) and the range's record bytes AT ONCE into a segment of exactly their size, as :class:`PipeSource` keeps a
        chunk's.  The first range the :class:`PipeStore` refuses opens the spool under the stream's own header, the kept records first;
        from then on every range's records are appended to it and nothing is kept; ``opened.pipe.store.mode`` says so to the caller."""
        pipe = opened.pipe
        store = pipe.on_device(dv, lambda: pipe.bam_header)
        chunks = textin.member_chunks(dv.torch, opened.text, range_bytes)
        for rng in index.stream_ranges(chunks, opened.head, opened.first, dv.dev, dv.clock, name=opened.path):
            part.range_reads += 1
            m = _bam_measured(dv, opened, part, rng)
            if m.length.size:
                need = int(m.length.sum())
                if store.admit(need):
                    part.drop_keys()
                d_seg = store.buffer(need)
                d_seg[:need].copy_(rng.d_raw[m.at:m.at + need])                 # the records that complete in the range: contiguous there
                store.keep(d_seg, need)
                del d_seg
            _keep_measured(part, rng.place, m, keys=store.spool is None)
            _release(rng)
            del rng, m
            dv.clock.lap("keep")
        opened.text.close()
        store.finish()


# ---- open ----
_COMPRESSED_SAM = ("%s: gzip- or BGZF-compressed data that is no BAM -- compressed SAM is not taken: decompress it, or convert it with "
                   "`samtools view -b`; through a pipe it is: `pigz -dc x.sam.gz | python -m svision_amd.sort - -o sorted.bam`")


def _open(path, alone=True, run=None):
    """open: -> Opened(the path, read_bam_header's table, first_record's (file offset, entry, references), the header's bytes as the
    output takes them, ``room``: the records' inflated bytes by the members' ISIZE fields) -- one pass over the file's members
    (index.bgzf_members, index.header_place).  SAM text (a first byte ``@``, or a first line of 11 tab-separated fields):
    :func:`_open_sam`; read once: :func:`_open_pipe`."""
    from .io import sam
    from .io.bam import read_bam_header
    if run is None and is_stream(path):
        raise SortWriteError("%s: not a regular file" % path)
    try:
        inp = textin.open_input(path)
    except (sam.SamError, OSError) as exc:
        raise SortWriteError("%s: %s" % (textin.name_of(path), exc)) from None
    if inp.kind != "bam":
        return _open_sam(inp, alone) if inp.kind == "sam" else _open_pipe(inp, alone, run)
    if inp.peek_kind == sam.STREAM_GZIP:
        raise SortWriteError(_COMPRESSED_SAM % path)
    try:
        head = read_bam_header(path)
        members = index.bgzf_members(path)
        place = index.header_place(path, members)               # (takes the members the header lies in; the rest follow below)
        header = sorted_header_bytes(place.head)
        room = place.isize + sum(isize for _at, _bsize, _xlen, isize in members) - len(place.head)
    except (ValueError, TypeError, OSError, zlib.error, struct.error) as exc:
        raise SortWriteError("%s: %s" % (path, exc)) from None
    if room < 0:
        raise SortWriteError("%s: its BGZF blocks hold fewer bytes than its header" % path)
    return Opened(path, head, tuple(place[:3]), header, room, BamSource())


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
                  SamSource() if pipe is None else PipeSource(), None, pipe, inp)


def _open_pipe(inp, alone, run):
    """open, an input that is read once, by what its first bytes hold (io.sam.stream_kind).

      SAM text  io.sam.StreamReader: the ``@`` lines are read up to the first line without ``@``; what was read beyond them stays in the
                reader's buffer: :func:`_open_sam`'s Opened, its source :class:`PipeSource`, the text waiting in the pipe
      a BAM     (``samtools view -b``, ``dorado aligner``, ``pbmm2``): BGZF or gzip magic whose inflated head is ``BAM\\1``.  By
                default the bytes are copied as they are into the spool file and the BAM road sorts that file -- one write and one read
                of compressed BAM more, room for it beside the output, and nothing runs on the device until the aligner has ended.
                Alone and under ``run.stream_bam``: its header read from the stream and the rest left waiting for :class:`BamPipeSource`
                -- unless the run has a :class:`TagFilter`: the filter is the BAM road's, so the copy is kept under either setting
      refused   other gzip data (compressed SAM: ``pigz -dc x.sam.gz | ... -`` is the road), no byte at all (``<stdin>: no input``)"""
    from .io import sam
    pipe = _Pipe(inp, run)
    run.pipes.append(pipe)
    refusal = {sam.STREAM_EMPTY: "%s: no input", sam.STREAM_GZIP: _COMPRESSED_SAM, sam.STREAM_OTHER: "%s: neither SAM text nor a BAM"}
    if inp.peek_kind in refusal:
        raise SortWriteError(refusal[inp.peek_kind] % inp.name)
    if inp.peek_kind == sam.STREAM_SAM:
        return _open_sam(inp, alone, pipe)
    pipe.holds = "bam"
    if alone and run.stream_bam and run.tags is None:          # (a tag filter works on the copy: the BAM road, under either setting)
        try:
            got = inp.reader.bam_header()
            pipe.bam_header = got.head
            return Opened(inp.name, got.table, got.first, sorted_header_bytes(got.head), None, BamPipeSource(), None, pipe, inp)
        except (sam.BgzfStreamError, ValueError, struct.error) as exc:
            raise SortWriteError("%s: %s" % (inp.name, exc)) from None
    pipe.store.mode = "bam_spooled"
    try:
        pipe.store.spool_file, pipe.store.spool_bytes = spool_copy(inp.reader, run.out_path, run.clock, pipe.number)
    except OSError as exc:
        raise SortWriteError("%s: %s" % (inp.name, exc)) from None
    inp.close()
    return _open(pipe.store.spool_file, alone)._replace(pipe=pipe)


def _pipe_spooled(dv, opened, header):
    """A pipe among several inputs is spooled from its first byte (``room`` is decided behind all key passes, and a pipe cannot be asked
    again), against the merged names and under the merged ``header``: its text through :meth:`PipeSource.key_pass` into the spool file
    -> the Opened of that file, a BAM like any other: the pipe is that file from ``_open_all`` on.  Its place in the list decides ties; without @SQ lines it is usable beside parts
    that have them.  ``-`` may appear once; further pipes of a run (FIFOs) spool to ``.spool.<pid>.<number>.bam`` and
    ``stats["pipes"]`` lists them all."""
    opened.source.key_pass(dv, opened, opened.pipe.run.range_bytes, SamPass(), None, header)
    return _open(opened.pipe.store.spool_file, alone=False)._replace(pipe=opened.pipe)
