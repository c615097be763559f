"""Device-side BAM ingestion (the default engine, svision_amd.ingest.ChromosomeFeed): the compressed file goes to the GPU as
it is -- through a ring of pinned 64 MB slots --, the BGZF blocks are inflated there (svx_bgzf_inflate_fast_on: parallel Huffman
decoding per block, then the LZ copies; the round-3 kernels by name: SVX_INFLATE_VARIANT), the CRC32 of every block is checked,
the records are located through
the .bai linear index and their fixed fields, QNAMEs and CIGAR words are packed on the device (svx_bam_walk_*).  The packed
CIGARs -- the input of svx_cigar_scan -- never leave HBM; the host receives the small per-record arrays its collection step
needs and hands them to the helper processes by WRITING them to shared-memory files (it never maps them: DESIGN.md section 5).

Why: DEFLATE decoding is the cost of ingestion (a HiFi BAM inflates to ~22 KB per read, ~0.6 GB/s per host core), and the
GPU boxes this was built on give a container the CPU time of 16 cores (svision_amd.ingest.effective_cpus): ~10 GB/s of
inflated data, a quarter of what the device pipeline consumes.  The same data inflates at 75 GB/s on the MI355X (two kernels,
136 and 170 GB/s).
Replaces pysam's AlignmentFile.fetch (run_collection.py:23-26) like the host reader (io.bam.BamStream), which stays the
engine for files without a linear index and for SVX_INGEST=cpu.  --hash / --graph want the read bases too: with
``with_seq`` the walk also packs every record's 4-bit SEQ (svx_bam_walk_*_seq); like the CIGAR words the bases stay in HBM until
the hand-over is through and follow through the spill thread (LazySeq, spill_seq).

Map of a run (DeviceDecoder.units_pipelined -> _Pipeline; the streams are those of svision_amd/streams.py):

  planning   the caller's thread: plan_units / whole_units -> Units (file ranges), cut_groups -> the groups, one inflate
             launch each.  No device work.
  reader     thread "svx-read" (_Pipeline.reader, read_group): one native call per group (svx_stage_group, csrc/svx_stage.hip) --
             a pool of pread threads, alive from run()'s start to its end, reads ahead into the staging ring, across groups;
             per slot the BGZF block index and the copy to the device on the "copy" stream --, then the record starts from the
             linear index.  (SVX_STAGE_READER=py: read, index, enqueue slot by slot in Python.)          -> Queue(maxsize=1)
  driver     thread "svx-inflate-driver" (drive, pump, launch, finish_group): inflate, CRC32, walk-count, then per unit the
             extraction and its read-back, on "ingest0" / "ingest1" in turn -- the tokens kernel of every group on "tokens"
             --; the large buffers are allocated on the thread's default stream.  (Thread "svx-inflate-warm": the first two
             groups' buffers, allocated and freed ahead of time.)                                      -> Queue(maxsize=8)
  consumer   the caller's thread (_Pipeline.run): (unit, finish, device arrays); finish() is host work (QNAME ids, table); the
             caller scans on a stream of its own, behind the unit's read-back event.
"""
import collections
import os
import queue
import threading
import time

import numpy as np
import torch

from . import _lib, kernels, streams
from .io.bam import AlignmentTable
from .io.csi import spans as index_spans, voff_at        # noqa: F401 -- (voff_at: the .bai look-up, part of this module's interface)

FIRST_GROUP_BYTES = 192 << 20            # the first launch is small (~7 k blocks): the pipeline starts after ~0.1 s
STAGE_BYTES = 64 << 20                   # a pinned staging slot of the reader (_StagingRing: eight of them)
PIPE_GROUP_BYTES = 400 << 20             # the SECOND group: two slices (~14 k blocks) -- a ramp 192 / 400 / 600 MB.  Round 6, measured (profiles/r06_group_sweep.txt):
                                         # the five-window chr21 job (BASELINE configs[1]) is cut [1, 2, 2] instead of [1, 4] and takes 0.142 s instead of 0.172
                                         # (its second and third window no longer wait for the inflate of all four); 20 windows, cfg1, ONT: unchanged (+-1 %)
                                         # The groups behind the first two: ~21 k blocks.  (Round 3 / early round 4: 768 MB, then 2.5 GB
LARGE_GROUP_BYTES = 600 << 20            # -- a launch of the lane-per-block kernel cost 60-90 ms whatever it held.  The two-kernel inflate is
LARGE_GROUP_BLOCKS = 94_000              # proportional to the launch, and once the read-backs no longer blocked each other (launch(), streams.py)
                                         # a steady flow of small groups beat the large ones: the CNN behind never runs out of chromosomes.  With the table LZ kernel --
                                         # no 25 ms floor per launch -- the sizes were swept again, profiles/lz_table.txt: nothing beat them by more than the spread.)
GROUP_BYTES = 24 << 30                   # read by no code of the package any more (the serial decoder it sized is gone): tests/test_gpu_inflate.py saves and restores it with the other sizes
SLICE_BYTES = 256 << 20                  # a chromosome is handed over in slices of whole collection windows of about this many compressed bytes
MIN_MARGIN = 128 << 10                   # reference bases a slice's records reach beyond its windows on either side, at least (plan_units)

_REACH_CACHE = {}                                             # (file identity) -> DeviceDecoder.estimate_reach: ~7 ms of zlib, once per file and process


class DeviceIngestError(RuntimeError):
    """``tids``: the references the failure belongs to (None: unknown -- the reference the consumer waits for is blamed)."""
    tids = None

    def __init__(self, msg, tids=None):
        super().__init__(msg)
        self.tids = list(tids) if tids is not None else None


class _LazyArray:
    """An array of a device-decoded table that exists on the device only at the hand-over and reaches the host a little
    later, through the spill thread.  ``attach(array)`` (owner process, after the spill) or ``path`` + ``ready`` (helper
    processes: the file the owner spills to and its completion flag)."""
    dtype, what = None, "array"

    def __init__(self, n, path=None, ready=None):
        self.size, self.nbytes, self.path, self.ready, self._arr = int(n), np.dtype(self.dtype).itemsize * int(n), path, ready, None
        self.event = None                    # owner process: set when the spill of this table is through (ingest.ChromosomeFeed)

    def attach(self, arr):
        self._arr = arr

    def _get(self):
        if self._arr is None:
            if self.path is None:
                # the owner process itself reads the array (-t 1: the by-value comparison of duplicated records, the k-mer
                # re-aligner's bases): the spill runs right behind the hand-over on a thread of its own -- wait for it (round 6:
                # with the hand-over 10 ms earlier the first window's collection could get here first, and the window was skipped
                # as "failed")
                if self.event is not None:
                    self.event.wait(timeout=120)
                if self._arr is not None:
                    return self._arr
                raise RuntimeError("the %s of this table are on the device only" % self.what)
            t0 = time.time()
            while not os.path.exists(self.ready):              # the owner spills them right after the hand-over
                if time.time() - t0 > 120:
                    raise RuntimeError("the spill %s never completed" % self.path)
                time.sleep(0.001)
            self._arr = np.memmap(self.path, dtype=self.dtype, mode="r", shape=(self.size,)) if self.size else np.empty(0, self.dtype)
        return self._arr

    def __getitem__(self, key):
        return self._get()[key]

    def __len__(self):
        return self.size

    def __array__(self, dtype=None, copy=None):
        a = self._get()
        return np.asarray(a, dtype) if dtype is not None else np.asarray(a)


class LazyCigar(_LazyArray):
    """Stand-in for ``AlignmentTable.cigar`` while the words exist on the device only."""
    dtype, what = np.uint32, "CIGAR words"


class LazySeq(_LazyArray):
    """Stand-in for ``AlignmentTable.seq_packed`` (``with_seq``) while the bases exist on the device only: the 4-bit SEQ bytes
    of every record, record i at byte ``seq_off[i]`` (AlignmentTable.query_sequence and subset take it as it is)."""
    dtype, what = np.uint8, "read bases"


class _PrivateSlot:
    """The private-memory twin of a shared-memory slot (ingest._Slot) for a decoder that serves no helper processes
    (``DeviceDecoder(take_slot=None)``): ``put`` keeps the array, nothing is written and no flag is set."""
    dir = None

    def put(self, _name, src):
        return np.ascontiguousarray(src).reshape(-1)

    def open_for(self, _name, _nbytes):
        return open(os.devnull, "wb")

    def mark(self, _flag):
        pass


def spill_cigar(table):
    """Owner process, off the critical path: the device CIGAR words of a device-decoded table -> this process's memory
    (LazyCigar.attach) and the table's slot; the file first, the flag the helper processes wait for (LazyCigar._get) behind it."""
    d_cigar, slot, lazy = table._d_cigar, table._slot, table.cigar
    host = np.empty(lazy.size, np.uint32)
    if lazy.size:
        torch.from_numpy(host.view(np.int32)).copy_(d_cigar[:lazy.size])
    lazy.attach(slot.put("cigar", host))
    slot.mark("cigar.ready")


SPILL_STAGE_BYTES = 8 << 20              # spill_seq: two pinned buffers of this size, whatever a group's bases come to (a third of its inflated bytes)
_SPILL_STAGE = []                        # (pinned tensor, event of its last copy) x 2, per process: the spill thread is the only user


def spill_seq(table):
    """Owner process, off the critical path, behind :func:`spill_cigar`: the device bases of a table decoded ``with_seq`` ->
    this process's memory (LazySeq.attach) and the slot's ``seq_packed.bin`` + the flag ``seq.ready``.  The copy goes
    through two pinned staging buffers of SPILL_STAGE_BYTES in turn -- the device-to-host copy of one chunk runs while the
    chunk before is written -- on the current stream."""
    d_seq, slot, lazy = table._d_seq, table._slot, table.seq_packed
    n = lazy.size
    host = np.empty(n, np.uint8)
    while len(_SPILL_STAGE) < 2:
        _SPILL_STAGE.append(torch.empty(SPILL_STAGE_BYTES, dtype=torch.uint8, pin_memory=True))
    chunks = [(at, min(SPILL_STAGE_BYTES, n - at)) for at in range(0, n, SPILL_STAGE_BYTES)]
    events = [None, None]

    def issue(i):
        at, m = chunks[i]
        _SPILL_STAGE[i % 2][:m].copy_(d_seq[at:at + m], non_blocking=True)
        events[i % 2] = torch.cuda.Event()
        events[i % 2].record()
    if chunks:
        issue(0)
        with slot.open_for("seq_packed", n) as f:
            for i, (at, m) in enumerate(chunks):
                if i + 1 < len(chunks):
                    issue(i + 1)
                events[i % 2].synchronize()
                part = _SPILL_STAGE[i % 2].numpy()[:m]
                host[at:at + m] = part
                f.write(part)
    lazy.attach(host)
    slot.mark("seq.ready")                                      # the flag the helper processes wait for (LazySeq._get)


class Unit:
    """What the decoder hands over in one piece: the records of reference ``tid`` that the collection windows [lo, hi) of the
    job can touch -- every record overlapping [lo - reach, hi + reach), reach = the longest alignment's span + the longest
    read + 1000 (sample.Sample.reach: cluster extents, the coverage count and the genotyper's +-1000 bp stay inside) -- as
    the file range [vlo, vhi) of virtual offsets, both ends at linear-index entries (or the ends of the reference's records).
    A whole chromosome is one unit with lo = 0, hi = its length.  ``left_edge``: every record that reaches beyond this
    coordinate lies at or behind ``vlo`` (None: vlo is the reference's first record)."""
    __slots__ = ("tid", "lo", "hi", "vlo", "vhi", "left_edge", "to_end", "first", "last", "windows")

    def __init__(self, tid, lo, hi, vlo, vhi, left_edge=None, to_end=True, first=True, last=True, windows=None):
        self.tid, self.lo, self.hi, self.vlo, self.vhi = int(tid), int(lo), int(hi), int(vlo), int(vhi)
        self.left_edge, self.to_end, self.first, self.last = left_edge, bool(to_end), bool(first), bool(last)
        self.windows = list(windows) if windows is not None else [(self.lo, self.hi)]

    def __repr__(self):
        return "Unit(tid %d, [%d, %d)%s%s)" % (self.tid, self.lo, self.hi, "" if self.left_edge is None else ", records from %d" % self.left_edge,
                                                 "" if self.to_end else ", cut")


def cut_groups(tids, size_of, first_limits, limit, merge_last=True):
    """Chromosomes in file order -> the groups whose blocks are inflated in one launch: the first groups of at most
    ``first_limits`` compressed bytes (the very first is small: the pipeline behind starts after one short launch), the others of at
    most ``limit``; a chromosome larger than its limit is a group of its own.  The two-kernel inflate is proportional to the launch
    and the read-backs of the groups no longer block each other, so a steady flow of small groups keeps the CNN behind supplied
    (the lane-per-block era made them as large as the chip: a launch cost 60-90 ms whatever it held).  ``merge_last``: a remainder
    of at most half a group joins the group in front of it -- launched on its own it is the last launch of the job, its LZ copies
    (latency-bound) run next to a CNN that has its full backlog by then (3-4 x slower than alone: 100 ms for 7 k blocks), and
    everything waits for that one chromosome."""
    groups, cur, cur_bytes = [], [], 0
    for t in tids:
        lim = first_limits[len(groups)] if len(groups) < len(first_limits) else limit
        if cur and cur_bytes + size_of(t) > lim:
            groups.append(cur)
            cur, cur_bytes = [], 0
        cur.append(t)
        cur_bytes += size_of(t)
    if cur:
        groups.append(cur)
    # (round 6: a QUARTER of a group, half until then -- with the LZ launches of round 5 a remainder of a third to a half of a group is
    # better off on its own: cfg1's [1, 2, 3, 2] slices per launch take 0.193 s, [1, 2, 5] 0.210; profiles/r06_group_sweep.txt)
    if merge_last and len(groups) > 2 and sum(size_of(t) for t in groups[-1]) * 4 <= limit:
        groups[-2:] = [groups[-2] + groups[-1]]
    return groups


def _size_of(unit):
    """Compressed bytes of a unit's file range, its last block included."""
    return (unit.vhi >> 16) - (unit.vlo >> 16) + 65536


_Blocks = collections.namedtuple("_Blocks", "k src_off src_len isize coff used")


def _index_blocks(lib, ptr, nbytes, file_offset):
    """svx_bgzf_index over the ``nbytes`` at host address ``ptr``, which lie at ``file_offset`` of the file -> _Blocks: ``k``
    whole BGZF blocks (negative: no block starts at ``ptr``), per block its payload's offset from ``ptr``, the payload's
    length, ISIZE and the block's file offset -- cut to ``k`` --, and ``used``: the bytes those blocks take."""
    cap = nbytes // 28 + 16
    src_off, coff = np.empty(cap, np.uint64), np.empty(cap, np.uint64)
    src_len, isize = np.empty(cap, np.uint32), np.empty(cap, np.uint32)
    used = np.zeros(1, np.uint64)
    k = int(lib.svx_bgzf_index(ptr, nbytes, file_offset, cap, src_off.ctypes.data, src_len.ctypes.data, isize.ctypes.data, coff.ctypes.data,
                               used.ctypes.data))
    n = max(k, 0)
    return _Blocks(k, src_off[:n], src_len[:n], isize[:n], coff[:n], int(used[0]))


def _record_starts(coff, dst, lo, hi, linear):
    """Where a walk of the records in the virtual-offset range [lo, hi) may start: ``lo``, the entries of the reference's
    linear index inside the range and ``hi``, as ascending offsets into the inflated bytes of blocks that lie at the file
    offsets ``coff`` and inflate to ``dst[i]`` .. ``dst[i + 1]`` (a virtual offset behind the last block: the end of the
    data; two virtual offsets of one byte -- a block boundary -- are one start)."""
    nb = int(coff.size)
    seeds = linear[(linear >= np.uint64(lo)) & (linear < np.uint64(hi))]
    voffs = np.unique(np.concatenate([np.asarray([lo], np.uint64), seeds, np.asarray([hi], np.uint64)]))
    c = voffs >> np.uint64(16)
    idx = np.searchsorted(coff, c)
    at_end = idx >= nb
    idx = np.minimum(idx, nb - 1)
    if not (at_end | (coff[idx] == c)).all():
        raise DeviceIngestError("the index points between two BGZF blocks")
    return np.unique(np.where(at_end, dst[nb], dst[idx] + (voffs & np.uint64(0xFFFF))))


def _pack_layout(n, name_bytes, with_seq=False):
    """-> (offs, size): the packed arrays of ``n`` records, everything the host wants of them, as sections of one buffer --
    [cig_off n+1][name_off n+1][tid n][pos n][l_seq n][flag n][mapq n][names] (8, 8, 4, 4, 4, 2, 1, 1 bytes an element) and,
    ``with_seq``, [seq_off n+1] (8) behind them (small: it goes with the hand-over; the bases themselves do not) --,
    section k at ``offs[k]``, each padded to 16 bytes, 16 more at the end and ``size`` a multiple of 256."""
    sect = [8 * (n + 1), 8 * (n + 1), 4 * n, 4 * n, 4 * n, 2 * n, n, name_bytes] + ([8 * (n + 1)] if with_seq else [])
    offs = np.zeros(len(sect) + 1, np.int64)
    offs[1:] = np.cumsum([(v + 15) // 16 * 16 for v in sect])
    return offs, (int(offs[-1]) + 16 + 255) // 256 * 256


def _section(d_pack, offs, k, dtype, count):
    """Section ``k`` of a device pack buffer (:func:`_pack_layout`) as ``count`` elements of the torch ``dtype``."""
    return d_pack[int(offs[k]):int(offs[k]) + count * torch.empty(0, dtype=dtype).element_size()].view(dtype)


class DeviceDecoder:
    def __init__(self, path, index, references, lengths, header_text, device, threads=8, take_slot=None, with_seq=False):
        self._t0, self.trace = time.perf_counter(), []          # (seconds since construction, what) of the first events (SVX_TIMING)
        self.path, self.references, self.lengths, self.header_text = path, list(references), list(lengths), header_text
        self.device, self.threads = torch.device(device), max(1, int(threads))
        self.take_slot = take_slot or _PrivateSlot               # callable() -> the slot of the next part (ingest._SlotPool.take: shared memory)
        self.with_seq = bool(with_seq)                           # the walk also packs the read bases (svx_bam_walk_*_seq): tables with seq_off + a LazySeq
        self.lib = _lib.load()
        # per reference None or its span in the index, .bai (LinearSpan) or .csi (CsiSpan): lo, hi, seeds, from_voff, to_voff
        self.spans = index_spans(index, decoder=True)
        self.size = os.path.getsize(path)
        self.stats = {"read_s": 0.0, "h2d_inflate_s": 0.0, "walk_s": 0.0, "d2h_s": 0.0, "names_s": 0.0, "blocks": 0, "bytes_in": 0, "bytes_inflated": 0}
        self._mark("index read")

    def _mark(self, what):
        if len(self.trace) < 400:
            self.trace.append((round(time.perf_counter() - self._t0, 4), what))

    def usable(self, tids):
        return self.unusable(tids) is None

    def unusable(self, tids):
        """Why the index does not serve the device engine for ``tids``, or None where it does."""
        for t in tids:
            if t >= len(self.spans):
                return "the index has %d references, the run wants reference %d" % (len(self.spans), t)
            span = self.spans[t]
            if span is not None and not span.usable:
                return ("the .csi has min_shift %d: the device engine cuts its slices at 16 kb windows (min_shift 14)" % span.min_shift
                        if hasattr(span, "min_shift") else "the .bai has no linear index for reference %d" % t)
        return None

    def _with_records(self, tids):
        """The references of ``tids`` that have records, in file order."""
        return [t for _v, t in sorted((self.spans[t][0], t) for t in tids if t < len(self.spans) and self.spans[t] is not None)]

    def whole_units(self, tids):
        """One unit per reference that has records, in file order: whole chromosomes."""
        return [Unit(t, 0, self.lengths[t] if t < len(self.lengths) else 1 << 62, self.spans[t][0], self.spans[t][1]) for t in self._with_records(tids)]

    def plan_units(self, tids, windows_of=None, margin=None, slice_bytes=None, resume=None, min_span_margins=None):
        """The references of ``tids`` that have records, in file order, each cut into slices of whole collection windows:
        ``windows_of(tid)`` -> its windows [(start, end), ...] ascending (None / a single window: the whole reference is one
        unit).  A slice is a run of windows of about ``slice_bytes`` compressed bytes (at least one window) and reads the
        records from the linear-index entry of ``start - margin`` to that of ``end + margin``: a real 30x chromosome is 3 GB
        of file, and its first window should not wait for all of it (the reference fetches window by window,
        run_collection.py:23-26).  ``margin`` is a guess (:meth:`estimate_reach`); the consumer checks every slice against the
        reach of its own records (ingest.ChromosomeFeed._reject -> planned again with a larger one).  ``resume`` = (tid,
        coordinate): leave out that reference's windows in front of the coordinate and every reference in front of it."""
        margin = int(margin if margin is not None else self.estimate_reach(tids))
        slice_bytes = int(slice_bytes or int(os.environ.get("SVX_SLICE_BYTES", "0")) or SLICE_BYTES)      # (the variable: experiments, tests)
        min_span = int(os.environ.get("SVX_SLICE_MIN_MARGINS", "13") if min_span_margins is None else min_span_margins) * margin
        units, skipping = [], resume is not None
        for t in self._with_records(tids):
            span = self.spans[t]
            wins = windows_of(t) if windows_of is not None else None
            wins = sorted((int(a), int(b)) for a, b in wins) if wins else None        # (a reference the job names no window of: whole)
            if skipping:
                if t != resume[0]:
                    continue
                skipping = False
                if wins is not None:
                    wins = [w for w in wins if w[1] > resume[1]]
                    if not wins:
                        continue
            if wins is None or os.environ.get("SVX_SLICES", "1") == "0":
                units.append(Unit(t, 0, self.lengths[t], span[0], span[1]))        # the whole chromosome (a resumed one: what is left of it is served by it)
                continue
            # a slice reads its margins twice (once with each neighbour): behind the reference's first slice -- one window, whatever
            # it costs: the pipeline waits for it -- a slice spans at least ~13 margins' worth of reference, so that long reads (ONT: a
            # margin of a megabase) do not turn a fifth of the file into overlap
            i = 0
            while i < len(wins):
                j = i + 1
                v0 = span.from_voff(wins[i][0])
                while j < len(wins) and (((span.to_voff(wins[j][1]) >> 16) - (v0 >> 16)) <= slice_bytes
                                         or (i > 0 and wins[j - 1][1] - wins[i][0] < min_span)):
                    j += 1
                lo, hi = wins[i][0], wins[j - 1][1]
                # (on the right TWICE the margin: the entry of a bin is the first record that overlaps it, which may start a whole read
                # length in front of it -- and the slice holds the records in front of THAT one.  A .csi's right end is a true upper
                # bound -- every record that starts in front of the coordinate is in --, yet the formula stays: the completeness check
                # goes by the slice's LAST record, which has to start behind what the windows need)
                vlo, vhi = span.from_voff(lo - margin), (span[1] if j == len(wins) and hi >= self.lengths[t] else span.to_voff(hi + 2 * margin))
                vhi = max(vhi, vlo)
                if vhi == vlo and vlo < span[1]:
                    # Both look-ups found the SAME record: either a coverage gap (it starts behind the slice) or ONE record that spans
                    # the whole slice, margins included (a small --window_size under a long read or contig) -- then it, and every
                    # record behind it that starts inside the windows, must not be dropped as "a slice without a record" (ADVICE r5).
                    # The slice takes the records up to the next entry of the index that lies behind this one: it is never empty
                    # here, and the consumer's completeness check (ChromosomeFeed._slice_complete) sees the spanning record.
                    vhi = span.next_behind(hi + 2 * margin, vlo)
                units.append(Unit(t, lo, hi, vlo, vhi, left_edge=None if vlo == span[0] else max(0, (lo - margin) >> 14 << 14), to_end=vhi == span[1],
                                  first=i == 0, last=j == len(wins), windows=wins[i:j]))
                i = j
        return units

    def estimate_reach(self, tids=None, sample=1 << 20, blocks=12):
        """A first guess of how far a slice must reach beyond its windows (:meth:`plan_units`): the records of a few 16 kb bins in
        the middle of the first reference are inflated on the host (zlib, a dozen blocks: ~9 ms) and walked -> the
        largest (reference span + read length) a log-normal fit of the sample expects among the reads crossing a window edge; at
        least MIN_MARGIN, a multiple of 16 kb.  Only a guess: reads are not of one length; every slice is checked against its own
        records afterwards."""
        if getattr(self, "_reach", None) is not None:
            return self._reach
        # (per file and process: a second pass over the same file -- a service, bench.py's legs behind its warm-up pass -- finds it)
        ident = (self.path, self.size, os.stat(self.path).st_mtime_ns, None if tids is None else min(tids, default=None))
        if ident in _REACH_CACHE:
            self._reach = _REACH_CACHE[ident]
            return self._reach
        import struct
        import zlib
        reach, logs = 0, []
        try:
            tid = min((s[0], t) for t, s in enumerate(self.spans) if s is not None and (tids is None or t in tids))[1]
            # (from the middle of the reference: the reads at its start are cut to it -- all of them short)
            v0 = self.spans[tid].from_voff(self.lengths[tid] // 2) if tid < len(self.lengths) else self.spans[tid][0]
            if v0 >= self.spans[tid][1]:
                v0 = self.spans[tid][0]
            start = v0 >> 16
            n = int(min(sample, self.size - start))
            buf = np.empty(n, np.uint8)
            if n > 0 and self.lib.svx_read_range(self.path.encode(), start, n, buf.ctypes.data, 1) == 0:
                raw, at, parts = buf.tobytes(), 0, []
                for _ in range(blocks):
                    if at + 18 > n or raw[at:at + 4] != b"\x1f\x8b\x08\x04":
                        break
                    xlen = struct.unpack_from("<H", raw, at + 10)[0]
                    bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1          # (htslib writes BC as the only extra subfield)
                    if at + bsize > n:
                        break
                    parts.append(zlib.decompress(raw[at + 12 + xlen:at + bsize - 8], -15))
                    at += bsize
                data = b"".join(parts)
                span_of = np.asarray([1, 0, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0], np.int64)
                p = v0 & 0xFFFF
                while p + 36 <= len(data):
                    size, _ref, _pos, l_name, _mq, _bin, n_cig, _flag, l_seq = struct.unpack_from("<iiiBBHHHi", data, p)
                    if size < 32:
                        break
                    if p + 36 + l_name + 4 * n_cig <= len(data):         # (the CIGAR is in hand although the record's bases may not be)
                        words = np.frombuffer(data, "<u4", n_cig, p + 36 + l_name)
                        each = int(((words >> 4).astype(np.int64) * span_of[words & 15]).sum()) + max(l_seq, 0)
                        reach = max(reach, each)
                        logs.append(np.log(max(each, 1)))
                    p += 4 + size
        except Exception:                                       # noqa: BLE001 -- a guess: the default stands
            reach, logs = 0, []
        # what a window needs beyond its edges is set by the longest of the reads that cross an edge -- a few dozen at 30 x, drawn
        # with a bias towards the long ones.  A log-normal fit of (reference span + read length) over the sample -- mu, sigma of the
        # logs -- puts the largest of ~60 length-biased draws near exp(mu + sigma^2 + 2.7 sigma): 1.4 x the median for reads of one
        # length (HiFi, sigma ~0.13), ~11 x for an ONT-like tail (sigma 0.7); never less than 1.25 x the largest seen.
        guess = 1.25 * reach
        if len(logs) > 3:
            mu, sg = float(np.mean(logs)), float(np.std(logs))
            guess = min(max(guess, float(np.exp(mu + sg * sg + 2.7 * sg))), 2.0 * reach)      # (a few dozen reads: the fit is kept within 1.25-2 x the largest)
        self._reach = max(MIN_MARGIN, (int(guess) + 1000 + 16383) >> 14 << 14)
        _REACH_CACHE[ident] = self._reach
        self._mark("reach guessed from a dozen blocks in mid-reference: %d" % self._reach)
        return self._reach

    def _block_bytes(self, tid, sample=1 << 20):
        """Mean size of a BGZF block in the file (a megabyte sampled at the start of reference ``tid``): the large groups are
        cut to the number of blocks one round of the lane-per-block kernel holds, whatever the file's compression ratio."""
        start = self.spans[tid][0] >> 16
        n = int(min(sample, self.size - start))
        if n <= 0:
            return 28_000.0
        buf = np.empty(n, np.uint8)
        if self.lib.svx_read_range(self.path.encode(), start, n, buf.ctypes.data, 1) != 0:
            return 28_000.0
        blocks = _index_blocks(self.lib, buf.ctypes.data, n, start)
        return float(blocks.used) / blocks.k if blocks.k > 0 else 28_000.0

    # ---- pipelined form: a reader thread, up to `depth` groups in flight on streams of their own ------------------------
    def parts_pipelined(self, tids, depth=2):
        """:meth:`units_pipelined` over whole chromosomes: yields (finish, device arrays) per reference that has records."""
        for _unit, finish, arrays in self.units_pipelined(self.whole_units(tids), depth):
            yield finish, arrays

    def units_pipelined(self, units, depth=2):
        """Generator over the units (:meth:`plan_units` / :meth:`whole_units`: whole chromosomes or slices of them, in file
        order): (unit, finish, (d_cigar int32, d_cig_off int64 [n+1], d_pos int32)) where ``finish()`` -> AlignmentTable on the
        host (the QNAME ids are computed there: host work the caller can overlap with the next unit's device work); (unit, None,
        None) for a unit without a record.  The steps are overlapped (:class:`_Pipeline`): a reader thread fills the device
        buffers of the groups ahead (through the staging ring); every group (cut_groups: ~600 MB of file) is inflated and
        counted without a host synchronisation -- its tokens kernel on the process's "tokens" stream, one group after the
        other, the rest on one of ``depth`` group streams (svision_amd/streams.py: hardware queues of their own) --; per group
        ONE read-back (block status + walk counts: issued when the inflate is through, never queued behind it), per unit ONE
        (the packed arrays).  Consecutive slices of one chromosome overlap by their margins: inside a group the overlap is
        inflated once (the group's bytes are one range of the file), across a group boundary twice (~2 % of a group)."""
        yield from _Pipeline(self, units, depth).run()

    def _make_finish(self, hp, n, words, name_bytes, d_cigar, seq_bytes=None, d_seq=None):
        """The host side of one device-decoded chromosome: packed read-back ``hp`` (:func:`_pack_layout`) -> shared-memory
        arrays, QNAME ids, table.  ``seq_bytes`` / ``d_seq`` (``with_seq``): the table gets its ``seq_off`` and a LazySeq over
        the bases, which are still on the device (``table._d_seq``: :func:`spill_seq`)."""
        lib = self.lib
        offs, _size = _pack_layout(n, name_bytes, seq_bytes is not None)

        def sect(k, dtype, count):
            return hp[int(offs[k]):int(offs[k]) + count * np.dtype(dtype).itemsize].view(dtype)

        def finish():
            t0 = time.perf_counter()
            slot = self.take_slot()

            # (what goes into the slot: views of the group's pinned read-back buffer, which lives as long as its views)
            cig_off_h = slot.put("cig_off", sect(0, np.int64, n + 1))
            name_off_h = sect(1, np.int64, n + 1)
            tid_h, pos_h, l_seq_h = slot.put("tid", sect(2, np.int32, n)), slot.put("pos", sect(3, np.int32, n)), slot.put("l_seq", sect(4, np.int32, n))
            flag_h, mapq_h = slot.put("flag", sect(5, np.uint16, n)), slot.put("mapq", sect(6, np.uint8, n))
            names_h = np.ascontiguousarray(sect(7, np.uint8, name_bytes))
            seq_off_h = slot.put("seq_off", sect(8, np.int64, n + 1)[:n]) if seq_bytes is not None else None      # (n entries, as the host decoder's)
            name_id = np.empty(n, np.int32)
            uniq = np.empty(max(name_bytes, 1), np.uint8)
            ub = np.zeros(1, np.uint64)
            name_off_c = np.ascontiguousarray(name_off_h)
            t1 = time.perf_counter()
            self.stats["finish_copy_s"] = self.stats.get("finish_copy_s", 0.0) + (t1 - t0)
            n_unique = int(lib.svx_name_ids(names_h.ctypes.data, name_off_c.ctypes.data, n, name_id.ctypes.data, uniq.ctypes.data, ub.ctypes.data))
            t2 = time.perf_counter()
            self.stats["finish_ids_s"] = self.stats.get("finish_ids_s", 0.0) + (t2 - t1)
            slot.put("name_id", name_id)
            blob = slot.put("names", uniq[:int(ub[0])].copy())
            name_list = blob.tobytes().decode().split("\n")[:-1] if n_unique else []
            self.stats["finish_list_s"] = self.stats.get("finish_list_s", 0.0) + (time.perf_counter() - t2)
            self.stats["names_s"] += time.perf_counter() - t0
            self._mark("finish(): slot copies + QNAME ids %.1f ms" % ((time.perf_counter() - t0) * 1e3))
            table = AlignmentTable(self.references, self.lengths, tid_h, pos_h, flag_h, mapq_h, l_seq_h, name_id, name_list, np.empty(0, np.uint32),
                                   cig_off_h, self.header_text)
            table.cigar = LazyCigar(words)
            table._slot = slot                                  # travels with the table: spill_cigar / spill_seq write to it
            table._d_cigar = d_cigar
            if seq_bytes is not None:
                table.seq_packed, table.seq_off, table._d_seq = LazySeq(seq_bytes), seq_off_h, d_seq
            return table
        return finish


class _Group:
    """One inflate launch: the units whose blocks it holds (one range of the file).  Filled by :meth:`_Pipeline.read_group`
    (reader thread), completed by :meth:`_Pipeline.launch` (driver thread: ``d_raw`` and everything behind it); the device
    buffers are dropped as soon as the last step that reads them is through."""
    __slots__ = ("units", "d_comp", "copied", "nbytes", "n_blocks", "inflated_bytes", "tab", "start_at", "n_starts",
                 "d_raw", "d_tab", "d_counts", "event", "stream")      # (d_counts, with_seq: the counts and, behind them, the SEQ bytes per start)

    def __init__(self, units, d_comp, copied, nbytes, n_blocks, inflated_bytes, tab, start_at, n_starts):
        self.units, self.d_comp, self.copied, self.nbytes, self.n_blocks, self.inflated_bytes = units, d_comp, copied, nbytes, n_blocks, inflated_bytes
        self.tab, self.start_at, self.n_starts = tab, start_at, n_starts      # pinned: block tables + every unit's record starts; where each unit's starts begin; how many
        self.d_raw = self.d_tab = self.d_counts = self.event = self.stream = None


class _Packed:
    """One unit's share of its group's pack buffers (:meth:`_Pipeline.finish_group`): where its record starts and walk counts
    are (``at`` in the group's table, ``n_starts`` rows from ``row``), what the walk counted (``n`` records, ``words`` CIGAR
    words, ``name_bytes``), its place in the buffers (``pack_at`` + ``size`` bytes laid out by ``offs``, ``word_at``) and, once
    its extraction is enqueued, what the consumer gets (``event``, ``h_pack``, ``d_cigar``, ``d_cig_off``, ``d_pos``)."""
    __slots__ = ("unit", "at", "n_starts", "row", "n", "words", "name_bytes", "offs", "pack_at", "size", "word_at",
                 "event", "h_pack", "d_cigar", "d_cig_off", "d_pos", "seq_bytes", "seq_at", "d_seq")

    def __init__(self, unit, at, n_starts, row, n, words, name_bytes, pack_at, word_at, seq_bytes=None, seq_at=0):
        self.unit, self.at, self.n_starts, self.row, self.n, self.words, self.name_bytes = unit, at, n_starts, row, n, words, name_bytes
        self.seq_bytes, self.seq_at = seq_bytes, seq_at          # with_seq: the SEQ bytes of the unit's records, their place in the group's buffer of bases
        self.offs, self.size = _pack_layout(n, name_bytes, seq_bytes is not None)
        self.pack_at, self.word_at = pack_at, word_at
        self.event = self.h_pack = self.d_cigar = self.d_cig_off = self.d_pos = self.d_seq = None


class _StagingRing:
    """The ring of pinned 64 MB slots a group's compressed bytes go to the device through -- read (8 pread threads), index the
    BGZF blocks the slot holds, copy them to their place in the group's device buffer on the copy stream, reuse the slot once
    its copy is done.  Eight slots (four, until round 4: a slot's "copy done" event sits in a hardware queue its stream shares
    with long kernels and completes tens of ms after the copy itself -- with four slots the reader waited 0.15 s of a 0.5 s job
    for slots whose copies had long finished, with eight 0.02 s; a stream with a hardware queue of its own -- one of the low
    priority class, which nothing else of the process uses -- changed nothing).  (First version: one pinned buffer per group in
    flight -- 3.7 GB of hipHostMalloc at 0.1 s per GB inside the run, during which every other HIP call of the process waited.)

    The slots outlive a decoder: a process that reads a second file (a service, a bench's warm-up pass) finds them allocated
    -- hipHostMalloc costs ~0.1 s per GB and every other HIP call of the process waits for it.  One decoder at a time owns the
    process-wide slots; another one running beside it gets a private ring."""
    _lock, _shared, _busy = threading.Lock(), [], False

    def __init__(self, stats):
        cls = _StagingRing
        with cls._lock:
            self.shared = not cls._busy
            if self.shared:
                cls._busy = True
        self.slots = cls._shared if self.shared else []        # [pinned tensor, "copy done" event of its last use or None]
        self.slots[:] = [s for s in self.slots if s[0].numel() == STAGE_BYTES]
        for s in self.slots:
            s[1] = None
        self.at, self.stats = 0, stats
        self.n_slots = max(2, int(os.environ.get("SVX_STAGE_SLOTS", "8")))

    def slot(self):
        """Reader thread -> the next slot, its previous copy complete (the wait is counted in stats["slot_wait_s"])."""
        if self.at < self.n_slots and len(self.slots) < self.n_slots:
            self.at += 1
            self.slots.append([torch.empty(STAGE_BYTES, dtype=torch.uint8, pin_memory=True), None])
            return self.slots[-1]
        s = self.slots[self.at % len(self.slots)]
        self.at += 1
        if s[1] is not None:
            t_w = time.perf_counter()
            s[1].synchronize()
            self.stats["slot_wait_s"] = self.stats.get("slot_wait_s", 0.0) + (time.perf_counter() - t_w)
        return s

    def pointers(self, n):
        """The native reader's view of the ring: the host addresses of its first ``n`` slots (at most ``n_slots``, at least two),
        allocated here where they do not exist yet.  The reader keeps an event per slot of its own; the torch events of
        :meth:`slot` are not used."""
        n = max(2, min(int(n), self.n_slots))
        while len(self.slots) < n:
            self.slots.append([torch.empty(STAGE_BYTES, dtype=torch.uint8, pin_memory=True), None])
        return [s[0].data_ptr() for s in self.slots[:n]]

    def release(self):
        """The process-wide slots are free for the next decoder (only once no thread of this one can touch them)."""
        if self.shared:
            with _StagingRing._lock:
                _StagingRing._busy = False


class _Pipeline:
    """One run of :meth:`DeviceDecoder.units_pipelined`: four threads, each stage a method.

        reader thread "svx-read"            reader -> read_group                 "copy" stream          -> Queue(maxsize=1)
        driver thread "svx-inflate-driver"  drive -> pump -> launch,             "ingest0" / "ingest1"  -> Queue(maxsize=8)
                                            drive -> finish_group                (+ "tokens", default)
        warm thread "svx-inflate-warm"      warm                                 default stream
        consumer (the caller's thread)      run

    The groups (module constants and SVX_*_GROUP_MB are read here, at call time) are cut before anything starts."""

    def __init__(self, dec, units, depth):
        self.dec, self.lib, self.dev, self.stats, self.mark = dec, dec.lib, dec.device, dec.stats, dec._mark
        units = list(units)

        def mb(name, default):                                 # (experiments: SVX_FIRST_GROUP_MB / SVX_PIPE_GROUP_MB / SVX_LARGE_GROUP_MB)
            v = os.environ.get(name)
            return int(v) << 20 if v else default
        large = mb("SVX_LARGE_GROUP_MB", LARGE_GROUP_BYTES)
        large = min(large, int(LARGE_GROUP_BLOCKS * dec._block_bytes(units[0].tid))) if units else large
        self.groups = cut_groups(units, _size_of, [mb("SVX_FIRST_GROUP_MB", FIRST_GROUP_BYTES), mb("SVX_PIPE_GROUP_MB", PIPE_GROUP_BYTES)], large,
                                 merge_last=os.environ.get("SVX_MERGE_LAST", "1") != "0")
        self.mark("groups cut: %s" % [len(g) for g in self.groups])
        self.read_q = queue.Queue(maxsize=1)                   # reader -> driver: _Group | None (the end) | an exception
        # The launches are driven from a thread of their own: the consumer of this generator does host work per chromosome
        # (QNAME ids, shared-memory copies, the upload for the scan: 3-80 ms) and a generator that launches only between two
        # of its yields left the device without inflate work for as long.
        self.out_q = queue.Queue(maxsize=8)                    # driver -> consumer: what run() yields | None | an exception
        self.stop = threading.Event()
        # (low class: the copies run on the DMA engines, and nothing else of the process uses that class's hardware queues: streams.py)
        self.copy_stream = streams.get("copy", self.dev)
        # high priority: the ingest kernels and the CNN share the device and do not overlap; whatever the order, the device
        # does the same work, but chromosomes that arrive early give the pipeline behind a backlog (and the per-chromosome
        # kernels here are small: behind queued graph replays they would wait for tens of ms)
        depth = int(os.environ.get("SVX_INGEST_DEPTH", depth))          # (experiments)
        self.depth = max(1, min(depth, 2))                         # (the high class has four hardware queues: tokens, two groups, scans)
        self.tokens_stream = streams.get("tokens", self.dev) if os.environ.get("SVX_TOKENS_STREAM", "1") != "0" else None
        self.group_streams = [streams.get("ingest%d" % i, self.dev) for i in range(self.depth)]
        self.inflight = collections.deque()                    # driver thread only: the groups launched and not yet finished
        self.n_read = 0                                        # reader thread only: groups read (read_group takes them in order, as the native reader does)
        self.done, self.error, self.launched = False, None, 0  # driver thread only: the reader has ended / what it ended with / groups launched
        # the file range of every group, whole BGZF blocks from the first unit's block to the last one's (its last block included)
        self.ranges = [(min(u.vlo >> 16 for u in g), min(dec.size, max(u.vhi >> 16 for u in g) + 65536 + 64)) for g in self.groups]
        # SVX_STAGE_READER=py: the per-slot loop in Python (read_slots_py), kept for A/B runs and as the tests' reference
        self.native = os.environ.get("SVX_STAGE_READER", "native") != "py"
        self.stage = None                                      # the native reader's handle (svx_stage_open), open inside run() only
        self.ring = _StagingRing(self.stats)                   # (last: from here on run()'s finally gives the shared slots back)

    # ---- reader thread ------------------------------------------------------------------------------------------------
    def reader(self):
        """Reader thread ("svx-read"): every group through :meth:`read_group`, then the end marker -- or the exception that
        ended it -- into ``read_q``.  Device work: the staging copies of read_group, on the "copy" stream."""
        def hand(item):                                         # stop-aware, the end marker and an exception included: an abandoned run
            while not self.stop.is_set():                       # (a failed group, a plan that is cut again) leaves nobody to take them,
                try:                                            # and a reader blocked for ever keeps the process-wide staging ring busy
                    self.read_q.put(item, timeout=0.2)
                    return True
                except queue.Full:
                    continue
            return False
        try:
            for g in self.groups:
                if not hand(self.read_group(g)):
                    return
            hand(None)
        except BaseException as exc:                             # noqa: BLE001
            hand(exc)

    def open_stage(self):
        """The caller's thread, inside :meth:`run`: the native reader over every group's file range and the ring's slots -- its
        pread pool starts on the first group at once.  (A slot is 64 KB of head-room + payload: svx_stage_core.hpp.)"""
        payload = STAGE_BYTES - 65536
        ptrs = self.ring.pointers(sum((c1 - c0 + payload - 1) // payload for c0, c1 in self.ranges))
        ranges = np.asarray(self.ranges, np.uint64).reshape(-1)
        slots = np.asarray(ptrs, np.uint64)
        index = self.dev.index if self.dev.index is not None else torch.cuda.current_device()
        self.stage = self.lib.svx_stage_open(self.dec.path.encode(), self.dec.threads, ranges.ctypes.data, len(self.ranges), slots.ctypes.data, len(ptrs),
                                             STAGE_BYTES, index, self.copy_stream.cuda_stream)
        if not self.stage:
            raise DeviceIngestError(self.lib.svx_bam_error().decode())

    def read_slots_native(self, d_comp, nbytes, tids_of):
        """Reader thread: ONE native call stages the group -- per slot it waits for the pool's bytes, indexes the BGZF blocks and
        enqueues the copy on the "copy" stream (svx_stage_group; the interpreter lock is released for the whole call) -- then
        the tables are copied out.  -> (src_off, src_len, isize, coff, copied)."""
        lib = self.lib
        cap = nbytes // (STAGE_BYTES - 65536) + 1
        used, waits, stamps = np.zeros(1, np.uint64), np.zeros(3, np.float64), np.zeros(2 * cap, np.float64)
        k = int(lib.svx_stage_group(self.stage, d_comp.data_ptr(), d_comp.numel(), used.ctypes.data, waits.ctypes.data, stamps.ctypes.data, cap))
        if k < 0:
            raise DeviceIngestError(lib.svx_bam_error().decode(), tids_of)
        with torch.cuda.stream(self.copy_stream):
            copied = torch.cuda.Event()
            copied.record()
        src_off, coff = np.empty(k, np.uint64), np.empty(k, np.uint64)
        src_len, isize = np.empty(k, np.uint32), np.empty(k, np.uint32)
        _lib.check(lib.svx_stage_tables(self.stage, src_off.ctypes.data, src_len.ctypes.data, isize.ctypes.data, coff.ctypes.data, k), "svx_stage_tables")
        self.stats["pread_s"] = self.stats.get("pread_s", 0.0) + float(waits[0])
        self.stats["slot_wait_s"] = self.stats.get("slot_wait_s", 0.0) + float(waits[1])
        n = int(np.count_nonzero(stamps[1::2]))
        if n:                                                   # (seconds since the reader was opened)
            self.mark("staged: %d slots, bytes of the first at %.4f, of the last at %.4f, last copy enqueued at %.4f" % (n, stamps[0], stamps[2 * n - 2], stamps[2 * n - 1]))
        return src_off, src_len, isize, coff, copied

    def read_slots_py(self, d_comp, c0, nbytes, tids_of):
        """Reader thread, SVX_STAGE_READER=py: slot by slot -- svx_read_range (threads started and joined per slot), svx_bgzf_index,
        the copy and the slot's torch event on the "copy" stream, then the next read.  -> (src_off, src_len, isize, coff, copied)."""
        dec, lib = self.dec, self.lib
        off, tables, copied = 0, [], None
        while off < nbytes:
            want = min(STAGE_BYTES, nbytes - off)
            slot = self.ring.slot()
            pin = slot[0]
            t_p = time.perf_counter()
            if lib.svx_read_range(dec.path.encode(), c0 + off, want, pin.data_ptr(), dec.threads) != 0:
                raise DeviceIngestError(lib.svx_bam_error().decode(), tids_of)
            self.stats["pread_s"] = self.stats.get("pread_s", 0.0) + (time.perf_counter() - t_p)
            blocks = _index_blocks(lib, pin.data_ptr(), want, c0 + off)
            if blocks.k < 0 or (blocks.k == 0 and off == 0):
                raise DeviceIngestError("no BGZF block at file offset %d" % (c0 + off), tids_of)
            if blocks.k == 0:
                break                                          # what is left of the range is the head of a block that ends behind it
            with torch.cuda.stream(self.copy_stream):
                d_comp[off:off + blocks.used].copy_(pin[:blocks.used], non_blocking=True)
                copied = torch.cuda.Event()
                copied.record()
            slot[1] = copied
            tables.append((blocks.src_off + np.uint64(off), blocks.src_len, blocks.isize, blocks.coff))
            off += blocks.used                                 # (a block cut by the end of the slot is read again, at the head of the next one)
        src_off, src_len, isize, coff = (np.concatenate([t[i] for t in tables]) for i in range(4))
        return src_off, src_len, isize, coff, copied

    def read_group(self, units):
        """Reader thread: the file range of ``units`` -> a :class:`_Group` whose compressed bytes are on their way to the
        device.  Allocates ``d_comp`` on this thread's default stream; the copies out of the staging slots go to the "copy"
        stream (``copied``: the event behind the last one).  The host work: waiting for the staged slots (read_slots_native; or
        pread and BGZF block index here, read_slots_py), record starts, the pinned table.

        ``stats``: ``read_s`` = the time this thread spends in here; ``pread_s`` = of that, the time it waited for a slot's
        bytes (the pool reads ahead, so what is left is what the reads could not hide; py: the svx_read_range calls);
        ``slot_wait_s`` = the time it waited for a slot's earlier copy to leave it."""
        dec = self.dec
        tids_of = sorted({u.tid for u in units})
        c0, c1 = self.ranges[self.n_read]
        self.n_read += 1
        nbytes = c1 - c0
        t0 = time.perf_counter()
        self.mark("read %s: start" % units[:2])
        d_comp = torch.empty((nbytes + 31) // 16 * 16, dtype=torch.uint8, device=self.dev)
        if self.native:
            src_off, src_len, isize, coff, copied = self.read_slots_native(d_comp, nbytes, tids_of)
        else:
            src_off, src_len, isize, coff, copied = self.read_slots_py(d_comp, c0, nbytes, tids_of)
        d_comp.record_stream(self.copy_stream)
        nb = int(src_off.size)
        dst = np.zeros(nb + 1, np.uint64)
        dst[1:] = np.cumsum(isize.astype(np.uint64))
        starts = []
        for u in units:
            try:
                starts.append(_record_starts(coff, dst, u.vlo, u.vhi, dec.spans[u.tid][2]))
            except DeviceIngestError as exc:
                raise DeviceIngestError(str(exc), [u.tid]) from None
        # one pinned block of small tables: payload offsets, payload sizes, inflated offsets, then every chromosome's starts
        n_starts = [int(a.size) - 1 for a in starts]
        words = 3 * nb + 1 + sum(a.size for a in starts) + 8
        tab = torch.empty(words, dtype=torch.int64, pin_memory=True)
        tv = tab.numpy()
        tv[:nb] = src_off.view(np.int64)
        tv[nb:2 * nb] = src_len.astype(np.int64)
        tv[2 * nb:3 * nb + 1] = dst.view(np.int64)
        at, start_at = 3 * nb + 1, []
        for a in starts:
            tv[at:at + a.size] = a.view(np.int64)
            start_at.append(at)
            at += a.size
        self.stats["read_s"] += time.perf_counter() - t0
        self.stats["blocks"] += nb
        self.stats["bytes_in"] += int(nbytes)
        self.stats["bytes_inflated"] += int(dst[nb])
        self.mark("read: done, %d blocks" % nb)
        return _Group(units, d_comp, copied, nbytes, nb, int(dst[nb]), tab, start_at, n_starts)

    # ---- driver thread ------------------------------------------------------------------------------------------------
    def launch(self, g, stream):
        """Driver thread: inflate + CRC + walk-count of group ``g``, enqueued without a host synchronisation.  ``d_raw`` and the
        inflate's workspace are allocated on this thread's DEFAULT stream and handed over with record_stream; the tokens
        kernel of the "fast" variant goes to the "tokens" stream, everything else to ``stream`` ("ingest0" / "ingest1");
        ``g.event`` is recorded behind the last kernel.  No device-to-host copy is enqueued here."""
        lib, dev, nb, tokens_stream = self.lib, self.dev, g.n_blocks, self.tokens_stream
        self.mark("launch %s: start" % g.units[:2])
        # The group's large buffers -- the inflated bytes, the inflate's workspace -- are taken on THIS thread's (default)
        # stream and handed to the group's stream with record_stream: the caching allocator keeps its free blocks per
        # stream, so buffers allocated on the ingest streams (new ones every run) never met a cached block and were
        # hipMalloc'ed fresh -- 0.2 ms per GB on most boxes, 15 ms per GB on some: a 0.24 s stall in front of the
        # largest group's launch (two of nine bench runs).
        variant = kernels.inflate_variant_for(nb)
        # (readable up to the next multiple of 16 behind its last byte: the walk's aligned loads, include/svx.h)
        d_raw = torch.empty((max(g.inflated_bytes, 1) + 15) // 16 * 16, dtype=torch.uint8, device=dev)
        d_ws = kernels.inflate_workspace(lib, variant, g.inflated_bytes, nb, dev)
        # (the allocator may hand out a block that default-stream work freed and is still using: the group's streams
        # order themselves behind whatever the default stream holds at this point -- normally nothing)
        allocated = torch.cuda.Event()
        allocated.record(torch.cuda.default_stream(dev))
        if tokens_stream is not None:
            tokens_stream.wait_event(allocated)
        with torch.cuda.stream(stream):
            stream.wait_event(allocated)
            stream.wait_event(g.copied)                        # the last slot of the group's compressed bytes is on the device
            d_comp = g.d_comp
            d_comp.record_stream(stream)
            d_raw.record_stream(stream)
            if d_ws is not None:
                d_ws.record_stream(stream)
            d_tab = g.tab.to(dev, non_blocking=True)
            d_status = torch.zeros(nb, dtype=torch.int32, device=dev)
            d_len = d_tab[nb:2 * nb].to(torch.int32)
            st = kernels._stream_ptr(dev)
            # every group's tokens kernel on ONE stream, in launch order (include/svx.h, svx_bgzf_inflate_fast_on): two of them
            # side by side share the chip and finish together -- late; in a row, the first group's chromosomes are out a
            # whole tokens launch earlier and its LZ copies (latency-bound) run next to the second group's tokens
            if tokens_stream is not None and variant == "fast":
                for t_ in (d_comp, d_ws, d_tab, d_len, d_status):
                    t_.record_stream(tokens_stream)
            kernels.launch_inflate(lib, variant, d_comp.data_ptr(), d_tab.data_ptr(), d_len.data_ptr(), d_tab[2 * nb:].data_ptr(), nb,
                                   d_raw.data_ptr(), d_status.data_ptr(), g.inflated_bytes, dev, ws=d_ws,
                                   tokens_stream=tokens_stream if variant == "fast" else None)
            if kernels.bgzf_crc_wanted():                      # the footers' CRC32 (htslib checks it on every block): status 9 where one differs
                _lib.check(lib.svx_bgzf_crc32(d_raw.data_ptr(), d_tab[2 * nb:].data_ptr(), d_comp.data_ptr(), d_tab.data_ptr(), d_len.data_ptr(), nb,
                                              d_status.data_ptr(), st), "svx_bgzf_crc32")
            total_starts = sum(g.n_starts)
            with_seq = self.dec.with_seq
            # (with_seq: the SEQ bytes per start lie behind the counts, in the same buffer -- the group's ONE read-back stays one)
            d_flat = torch.empty(4 * (total_starts + 1) + (total_starts if with_seq else 0), dtype=torch.int64, device=dev)
            d_counts = d_flat[:4 * (total_starts + 1)].view(total_starts + 1, 4)
            row = 0
            for at, n in zip(g.start_at, g.n_starts):
                if with_seq:
                    _lib.check(lib.svx_bam_walk_count_seq(d_raw.data_ptr(), d_tab[at:].data_ptr(), n, d_counts[row:].data_ptr(),
                                                          d_flat[4 * (total_starts + 1) + row:].data_ptr(), st), "svx_bam_walk_count_seq")
                else:
                    _lib.check(lib.svx_bam_walk_count(d_raw.data_ptr(), d_tab[at:].data_ptr(), n, d_counts[row:].data_ptr(), st), "svx_bam_walk_count")
                row += n
            d_counts[total_starts, 0] = d_status.max()
            d_counts = d_flat
            # NO read-back is enqueued here.  A device-to-host copy goes to a DMA engine's queue at once, with a wait for
            # the kernels in front of it -- and the engine serves its queue in order: the counts' copy sat there for the
            # whole inflate (40-120 ms) and every other read-back of the process (the previous group's packed arrays,
            # the scans' results, the CNN's predictions) waited behind it.  finish_group() copies once the event is through.
            ev = torch.cuda.Event()
            ev.record()
        g.d_raw, g.d_tab, g.d_counts, g.event, g.stream = d_raw, d_tab, d_counts, ev, stream
        self.mark("launched %s" % g.units[:2])
        return g

    def finish_group(self, g):
        """Driver thread, generator: waits for ``g.event``, reads the counts back (the group's ONE read-back: on the group's
        stream, into pinned memory), enqueues every unit's extraction and packed read-back on the group's stream -- the two
        buffers they share are allocated on this thread's DEFAULT stream -- and yields None (everything is enqueued: the
        driver may launch the next group), then per unit what :meth:`run` yields, each after its own read-back event."""
        lib, dev, stream = self.lib, self.dev, g.stream
        t0 = time.perf_counter()
        g.event.synchronize()
        self.mark("inflate + count done %s" % g.units[:2])
        g.d_comp = None
        self.stats["h2d_inflate_s"] += time.perf_counter() - t0
        d_counts, g.d_counts = g.d_counts, None
        with_seq, total_starts = self.dec.with_seq, sum(g.n_starts)
        h_counts = torch.empty(tuple(d_counts.shape), dtype=torch.int64, pin_memory=True)
        with torch.cuda.stream(stream):
            h_counts.copy_(d_counts, non_blocking=True)
            ev_c = torch.cuda.Event()
            ev_c.record()
        ev_c.synchronize()
        counts = h_counts.numpy()[:4 * (total_starts + 1)].reshape(total_starts + 1, 4)
        seq_counts = h_counts.numpy()[4 * (total_starts + 1):]      # (with_seq: SEQ bytes per start)
        if int(counts[-1, 0]) != 0:
            raise DeviceIngestError("corrupt BGZF blocks in %s" % g.units, sorted({u.tid for u in g.units}))
        d_raw, d_tab = g.d_raw, g.d_tab
        t0 = time.perf_counter()
        # Sizes first, then ONE device buffer and ONE pinned buffer per group for the packed arrays of all its chromosomes
        # (and one device buffer for their CIGAR words): every first-time hipMalloc / hipHostMalloc of a run costs
        # milliseconds during which the other threads' HIP calls -- and their page faults -- wait; per chromosome that
        # was six of them.
        packed, row, pack_at, word_at, seq_at = [], 0, 0, 0, 0
        for unit, at, n_starts in zip(g.units, g.start_at, g.n_starts):
            c = counts[row:row + n_starts]
            bad = c[:, 3] != 0
            if bad.any():
                code = int(c[bad, 3][0])
                raise DeviceIngestError({1: "the linear index does not match the records", 2: "malformed BAM record"}.get(code, "walk error %d" % code), [unit.tid])
            n, words, name_bytes = (int(v) for v in c[:, :3].sum(axis=0)) if n_starts else (0, 0, 0)
            seq_bytes = int(seq_counts[row:row + n_starts].sum()) if with_seq else None
            p = _Packed(unit, at, n_starts, row, n, words, name_bytes, pack_at, word_at, seq_bytes, seq_at)
            packed.append(p)
            pack_at += p.size
            if with_seq:
                seq_at += (max(seq_bytes, 1) + 255) // 256 * 256
            word_at += (max(words, 1) + 63) // 64 * 64           # (svx_cigar_scan reads 16-byte quads: every chromosome starts aligned)
            row += n_starts
        rows = max(row, 1)
        base_flat = torch.zeros(3 * rows + (rows if with_seq else 0), dtype=torch.int64, pin_memory=True)      # (with_seq: the fourth base, behind the three)
        base_all, seq_base_all = base_flat.numpy()[:3 * rows].reshape(rows, 3), base_flat.numpy()[3 * rows:]
        for p in packed:
            if p.n_starts > 1:
                base_all[p.row + 1:p.row + p.n_starts] = np.cumsum(counts[p.row:p.row + p.n_starts - 1, :3], axis=0)
                if with_seq:
                    seq_base_all[p.row + 1:p.row + p.n_starts] = np.cumsum(seq_counts[p.row:p.row + p.n_starts - 1])
        d_pack_all = torch.empty(max(pack_at, 256), dtype=torch.uint8, device=dev)        # (default stream: see launch())
        d_cigar_all = torch.empty(max(word_at, 64), dtype=torch.int32, device=dev)
        # the group's bases: they stay here until the spill thread has copied them out (table._d_seq), never in the read-back below
        d_seq_all = torch.empty(max(seq_at, 256), dtype=torch.uint8, device=dev) if with_seq else None
        allocated = torch.cuda.Event()
        allocated.record(torch.cuda.default_stream(dev))
        with torch.cuda.stream(stream):
            stream.wait_event(allocated)
            st = kernels._stream_ptr(dev)
            d_pack_all.record_stream(stream)
            d_cigar_all.record_stream(stream)
            if with_seq:
                d_seq_all.record_stream(stream)
            d_base_flat = base_flat.to(dev, non_blocking=True)
            d_base_all = d_base_flat[:3 * rows].view(rows, 3)
            h_pack_all = torch.empty(max(pack_at, 256), dtype=torch.uint8, pin_memory=True)
            for p in packed:
                if p.n == 0:                                     # a slice (or a reference) without a record: nothing to extract
                    continue
                n = p.n
                d_pack = d_pack_all[p.pack_at:p.pack_at + p.size]
                d_base = d_base_all[p.row:p.row + p.n_starts]
                d_cig_off, d_name_off = _section(d_pack, p.offs, 0, torch.int64, n + 1), _section(d_pack, p.offs, 1, torch.int64, n + 1)
                d_tid, d_pos, d_lseq = _section(d_pack, p.offs, 2, torch.int32, n), _section(d_pack, p.offs, 3, torch.int32, n), _section(d_pack, p.offs, 4, torch.int32, n)
                d_flag, d_mapq = _section(d_pack, p.offs, 5, torch.int16, n), _section(d_pack, p.offs, 6, torch.uint8, n)
                d_names = _section(d_pack, p.offs, 7, torch.uint8, max(p.name_bytes, 1))
                d_cigar = d_cigar_all[p.word_at:p.word_at + max(p.words, 1)]
                if with_seq:
                    p.d_seq = d_seq_all[p.seq_at:p.seq_at + max(p.seq_bytes, 1)]
                    _lib.check(lib.svx_bam_walk_extract_seq(d_raw.data_ptr(), d_tab[p.at:].data_ptr(), p.n_starts, d_base.data_ptr(), d_tid.data_ptr(),
                                                            d_pos.data_ptr(), d_flag.data_ptr(), d_mapq.data_ptr(), d_lseq.data_ptr(), d_cig_off.data_ptr(),
                                                            d_cigar.data_ptr(), d_name_off.data_ptr(), d_names.data_ptr(),
                                                            d_base_flat[3 * rows + p.row:].data_ptr(), _section(d_pack, p.offs, 8, torch.int64, n + 1).data_ptr(),
                                                            p.d_seq.data_ptr(), n, st), "svx_bam_walk_extract_seq")
                else:
                    _lib.check(lib.svx_bam_walk_extract(d_raw.data_ptr(), d_tab[p.at:].data_ptr(), p.n_starts, d_base.data_ptr(), d_tid.data_ptr(),
                                                        d_pos.data_ptr(), d_flag.data_ptr(), d_mapq.data_ptr(), d_lseq.data_ptr(), d_cig_off.data_ptr(),
                                                        d_cigar.data_ptr(), d_name_off.data_ptr(), d_names.data_ptr(), n, st), "svx_bam_walk_extract")
                p.h_pack = h_pack_all[p.pack_at:p.pack_at + p.size]
                p.h_pack.copy_(d_pack, non_blocking=True)
                # svx_cigar_scan reads the offsets and positions where they are: views of the group's pack buffer, which
                # lives as long as one of them does (until round 4: two clones and two fills of the CSR arrays' closing
                # entries per chromosome -- four tiny launches, each a few hundred microseconds of waiting for room on a
                # chip that is full of inflate and CNN waves; the extract kernel writes the closing entries itself now).
                # The consumer scans on another stream and orders itself behind this one through the event only.
                p.event = torch.cuda.Event()
                p.event.record()
                p.d_cigar, p.d_cig_off, p.d_pos = d_cigar, d_cig_off, d_pos
        self.stats["walk_s"] += time.perf_counter() - t0
        yield None                                              # every chromosome's extraction is enqueued: the caller may launch the next group
        for p in packed:
            if p.event is None:
                yield p.unit, None, None
                continue
            t0 = time.perf_counter()
            p.event.synchronize()
            self.stats["d2h_s"] += time.perf_counter() - t0
            self.mark("packed read-back done")
            yield p.unit, self.dec._make_finish(p.h_pack.numpy(), p.n, p.words, p.name_bytes, p.d_cigar, p.seq_bytes, p.d_seq), (p.d_cigar, p.d_cig_off, p.d_pos)
        g.d_raw = g.d_tab = None

    def pump(self, block):
        """Driver thread: launch what the reader has ready, up to ``depth`` groups in flight, each on the next of the group
        streams; block only when nothing is in flight."""
        while not self.done and len(self.inflight) < self.depth:
            try:
                item = self.read_q.get(block=block and not self.inflight, timeout=None)
            except queue.Empty:
                return
            if item is None:
                self.done = True
                return
            if isinstance(item, BaseException):
                # a LATER group failed in the reader: the groups in flight in front of it are healthy -- they are finished and
                # their chromosomes yielded first (drive() raises this once nothing is in flight any more), so that the
                # consumer's count of finished chromosomes points at the failing group and nothing decoded is thrown away
                self.error, self.done = item, True
                return
            self.inflight.append(self.launch(item, self.group_streams[self.launched % self.depth]))
            self.launched += 1

    def put(self, x):
        """Driver thread: ``x`` into ``out_q`` unless the consumer has gone (-> False)."""
        while not self.stop.is_set():
            try:
                self.out_q.put(x, timeout=0.2)
                return True
            except queue.Full:
                continue
        return False

    def drive(self):
        """Driver thread ("svx-inflate-driver"): pump, wait for the oldest group in flight, finish it unit by unit into
        ``out_q`` -- pumping all the while --, then the end marker or the exception (the reader's, once nothing is in flight
        in front of it).  Issues no device work of its own: that is launch() and finish_group()."""
        try:
            while not self.stop.is_set():
                self.pump(block=True)
                if not self.inflight:
                    if self.error is not None:
                        raise self.error
                    break
                head = self.inflight[0]
                while not head.event.query():                  # keep launching while the oldest group is still on the device ...
                    self.pump(block=False)
                    time.sleep(0.0005)
                self.inflight.popleft()
                for part in self.finish_group(head):
                    # (None: the group's extraction is enqueued -- what is launched now runs behind it)
                    if part is not None and not self.put(part):
                        return
                    self.pump(block=False)                      # (a group of a dozen chromosomes takes tens of ms to finish)
                self.mark("group %s finished" % head.units[:2])
            self.put(None)
        except BaseException as exc:                             # noqa: BLE001 -- re-raised in the consumer's thread
            self.put(exc)

    # ---- warm thread --------------------------------------------------------------------------------------------------
    def warm(self):
        """Warm thread ("svx-inflate-warm"), default stream: the device buffers of the first two groups, allocated while the
        first read is still on its way (the caching allocator hands them out again): their hipMalloc calls would sit on the
        path to the first chromosome.  Only those: on some boxes a first hipMalloc costs 15 ms per GB instead of 0.2 -- 0.3 s
        for the 22 GB of all groups, during which no other HIP call of the process returns -- and the large groups' buffers
        are better allocated when their turn comes, next to device work that is already queued."""
        for g in self.groups[:2]:                              # in the order they will be asked for: compressed bytes, inflated bytes
            nbytes = sum(_size_of(u) for u in g)
            if self.stop.is_set():
                break
            for n in (nbytes + (1 << 20), 3 * nbytes + (1 << 20)):
                torch.empty(n, dtype=torch.uint8, device=self.dev)      # allocated and released at once: the block stays in the allocator's cache
        self.mark("warm: done")

    # ---- consumer -----------------------------------------------------------------------------------------------------
    def run(self):
        """The caller's thread, generator: starts the three threads and yields what the driver puts out; an exception of the
        reader or the driver is raised here.  No device work; on exit (exhausted, failed or abandoned) the threads are told
        to stop, the reader is joined and the "copy" stream synchronised before the native reader is closed (its pread pool exists
        between open_stage() here and that close only) and the staging slots go back."""
        reader = threading.Thread(target=self.reader, name="svx-read", daemon=True)
        started = False
        try:
            if self.native and self.groups:
                self.open_stage()
            reader.start()
            started = True
            threading.Thread(target=self.warm, name="svx-inflate-warm", daemon=True).start()
            threading.Thread(target=self.drive, name="svx-inflate-driver", daemon=True).start()
            while True:
                part = self.out_q.get()
                if part is None:
                    break
                if isinstance(part, BaseException):
                    raise part
                yield part
        finally:
            self.stop.set()
            try:
                if started:
                    reader.join(timeout=10)                    # (an abandoned run: the reader may be in the middle of a group)
                self.copy_stream.synchronize()                 # the slots go back to the process-wide ring: no copy may still read them
            finally:
                if not reader.is_alive():
                    if self.stage:                             # the pool is joined in here: no native thread outlives the run
                        self.lib.svx_stage_close(self.stage)
                        self.stage = None
                    self.ring.release()
