"""Chromosome-by-chromosome ingestion of a BAM file, overlapped with the pipeline.

The reference opens the BAM in every pool worker and fetches one window at a time (run_collection.py:23-26).  Here a rank's
chromosomes are streamed once, in file order; each part's packed arrays land in shared memory, are scanned on the device
(svx_cigar_scan) and are handed to the forked host helpers by name -- while the windows of the chromosome before are still in
the pipeline.  Nothing of the file other than the chromosomes in flight is resident.

Two feeds, one interface (``poll`` / ``get`` / ``release``):

  StaticFeed      a Sample that is already complete (tests, ``bench.py`` with the alignments resident in HBM)
  ChromosomeFeed  the file-driven one (the command line, ``bench.py --from-bam``)

Map of a ChromosomeFeed (each stage a method; a part travels as a :class:`_Part`, its arrays in a :class:`_Slot`):

  stage A   thread "svx-decode" (_decode -> _decode_device -> _device_pass, _settle, host_takes; _host_parts): the rank's chromosomes --
            whole (host engine: the native reader's threads, libdeflate) or in slices of collection windows (device engine:
            ingest_gpu.DeviceDecoder) -- decoded, their per-record arrays written to a slot.           -> Queue(maxsize=2)
  stage B   thread "svx-feed" (_run -> _accept, _scan, _reject, _hand_over), on the "scan" stream: QNAME ids, upload (host engine) +
            svx_cigar_scan, the check that a slice holds every record its windows can touch -- if not, stage A cuts the rest again
            (:class:`_Replan`) --, scan results into the slot, the meta.                               -> Queue(maxsize=depth)
  stage C   thread "svx-spill" (_spill), on the "spill" stream, device engine only: the CIGAR words and read bases of a part that has
            been handed over, device -> slot, each file in front of its ready flag.
  last      the owner thread (poll / get / take_fresh / release / close): parts into ``samples``, their metas to the helper processes
            (load_shared_sample maps the slot there), the slot back to the pool when the chromosome is done.
"""
import itertools
import logging
import os
import queue
import shutil
import tempfile
import threading
import time

import numpy as np

from .io.bam import AlignmentTable, BamStream
from . import streams
from .sample import Sample

# What "auto" means for a run that wants the read bases (--hash / --graph), decided by measurement (profiles/ingest_seq_ab.txt,
# DESIGN.md section 6): the device engine only if its median is below the host engine's fastest run.  An explicit
# engine="gpu" / SVX_INGEST=gpu is honoured either way.
AUTO_WITH_SEQ = "cpu"

_KEYS = itertools.count()                                    # keys of the parts announced to the helper processes (pipeline.PooledHotPath)


def effective_cpus():
    """CPUs this process can actually use: its affinity mask, capped by the cgroup's CPU-time quota (a container that
    sees 256 CPUs may be allowed the time of 16: more runnable threads than that get the whole group throttled for the
    rest of every scheduling period, the GPU-feeding thread included).  -> (usable CPUs, visible CPUs)."""
    visible = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:              # cgroup v2: "<quota> <period>" or "max <period>"
            q, period = f.read().split()[:2]
            if q != "max":
                quota = int(q) / int(period)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                q, period = int(f.read()), int(g.read())
                if q > 0:
                    quota = q / period
        except (OSError, ValueError):
            pass
    usable = visible if quota is None else max(1, min(visible, int(quota)))
    return usable, visible


def decode_threads(ranks_on_node=1, helpers=1):
    """Inflate threads of one rank: twice the node's usable CPUs divided by its ranks, at most 128.  The helpers wait for
    the decoder whenever it is the limit, so nothing is subtracted for them; a CPU-time quota is enforced per 100 ms period,
    and more runnable threads than CPUs use a period's budget earlier (measured on a 16-CPU quota, the same 9.3 GB of
    inflated data: 7 threads 2.2 s, 14 threads 1.11-1.4 s, 21 threads 1.05 s, 56 threads 0.95 s)."""
    usable, _visible = effective_cpus()
    return max(2, min(128, 2 * usable // max(ranks_on_node, 1)))


def empty_sample(references, lengths, fasta, min_sv, header_text=""):
    """A chromosome without records: its windows still exist as tasks (SVision:172-201) and yield nothing."""
    from . import kernels
    table = AlignmentTable(references, lengths, [], [], [], [], [], [], [], [], [0], header_text)
    return Sample.with_scan(table, fasta, min_sv, (np.empty(0, kernels.GAP_DTYPE), np.zeros(1, np.int64), np.empty((0, 4), np.int32)))


class StaticFeed:
    """Every chromosome is served by one resident Sample (key None: the helpers have it since their fork / attach_scan)."""

    def __init__(self, sample):
        self.sample = sample

    def poll(self, block=False):
        return False

    def take_fresh(self):
        return []

    def get(self, chrom, block=True, start=None):
        return None, self.sample

    def keys_of(self, chrom):
        return []

    def release(self, chrom):
        pass

    def close(self):
        pass


# ---- shared-memory slots -------------------------------------------------------------------------------------------
# A part's arrays live in the files of one slot directory; a released slot is handed to a later part and its files are
# overwritten in place: their pages stay allocated (a fresh tmpfs page costs a fault and a memset -- writing 270 MB of new
# files took 0.19 s, a sixth of a 20-window job).
class _Slot:
    """One slot directory.  Arrays are WRITTEN to its files and the caller keeps using its own copy -- no mapping is created in this process.
    np.memmap here cost the first file-driven pass of a process two stalls of 0.1-0.2 s: mmap() needs the address-space lock for writing, and
    while the process's first hipMalloc / hipHostMalloc calls and the runtime's page pinning hold it, the caller -- the one thread every
    chromosome passes through -- stood in mmap() (periodic stack dumps: numpy memmap.__new__, four in a row).  The helpers map the files in their
    own processes, which have no HIP runtime.  ``arrays``: {name: (dtype.str, n)} of what has been put, for the meta.  (Twin without files: ingest_gpu._PrivateSlot.)"""

    def __init__(self, d):
        self.dir, self.arrays = d, {}

    def open_for(self, name, nbytes):
        """``name``.bin opened for writing ``nbytes`` from its start: the file as it is when they fit, else re-created."""
        path = os.path.join(self.dir, name + ".bin")
        return open(path, "r+b" if os.path.exists(path) and os.path.getsize(path) >= nbytes else "wb")

    def put(self, name, src):
        """Record and write an array (an empty one is recorded only) -> the array, flat and contiguous."""
        src = np.ascontiguousarray(src).reshape(-1)
        self.arrays[name] = (src.dtype.str, int(src.size))
        if src.size:
            with self.open_for(name, src.nbytes) as f:
                f.write(src.view(np.uint8))
        return src

    def mark(self, flag):
        """Create the flag file the helper processes wait for (``cigar.ready`` / ``seq.ready``): behind the file it announces."""
        open(os.path.join(self.dir, flag), "w").close()


class _SlotPool:
    """The slot directories under ``root``: ``take()`` -> a _Slot on a released directory (its ready flags cleared, its files
    kept) or on a fresh one; ``give(dir)`` when the part is done with.  Any thread."""

    def __init__(self, root):
        self.root, self.lock, self.free, self.made = root, threading.Lock(), [], 0

    def take(self):
        with self.lock:
            d = self.free.pop() if self.free else None
            if d is None:
                d = os.path.join(self.root, "s%d" % self.made)
                self.made += 1
                os.makedirs(d)
        for flag in ("cigar.ready", "seq.ready"):
            if os.path.exists(os.path.join(d, flag)):
                os.remove(os.path.join(d, flag))
        return _Slot(d)

    def give(self, d):
        with self.lock:
            self.free.append(d)


# What a slot holds of a part, by file name: the table's arrays (host engine: put_table; device engine: ingest_gpu's
# finish() and, later, spill_cigar / spill_seq), then the scan's.  load_shared_sample reads through the same lists.
TABLE_ARRAYS = (("tid", np.int32), ("pos", np.int32), ("flag", np.uint16), ("mapq", np.uint8), ("l_seq", np.int32), ("name_id", np.int32),
                ("cig_off", np.int64), ("cigar", np.uint32), ("names", np.uint8))
SEQ_ARRAYS = (("seq_off", np.int64), ("seq_packed", np.uint8))
SCAN_ARRAYS = ("gaps", "gap_off", "stats")                   # (gaps: kernels.GAP_DTYPE, gap_off: int64, stats: int32 [n, 4])


def put_table(slot, table, with_seq):
    """A host-decoded table's arrays (io.bam.BamStream: private memory) -> the slot."""
    for name, _dtype in TABLE_ARRAYS + (SEQ_ARRAYS if with_seq else ()):
        slot.put(name, table._names_blob if name == "names" else getattr(table, name))


def part_meta(slot, table, sample, references, lengths, min_sv, with_seq):
    """The scan's arrays -> the slot; -> what a helper needs to map the part (load_shared_sample): a plain dict, it crosses a pipe."""
    for name in SCAN_ARRAYS:
        slot.put(name, getattr(sample, name))
    return {"dir": slot.dir, "arrays": dict(slot.arrays), "references": references, "lengths": lengths, "min_sv": min_sv, "n": len(table),
            "with_seq": with_seq, "header_text": table.header_text, "stats_shape": list(np.shape(sample.stats))}


# ---- slices: what a window needs, what a refused device pass leaves to the host ----------------------------------
def grow_margin(needed, margin):
    """The margin the slices are cut again with after one needed ``needed`` bases: twice that, at least twice the old one, in 16 kb bins."""
    return (max(2 * needed, 2 * margin) + 16383) >> 14 << 14


def host_takes(rest, tids, refusals):
    """After a DeviceIngestError (an index that does not fit, a corrupt block): the references the host reader takes over -- whole;
    what the device has handed over of them stays, the host's table serves the rest -- given ``rest`` (the units not handed over yet),
    ``tids`` (those the error names; None or none of ``rest``: the one the consumer waits for is blamed) and ``refusals`` (this one
    included): everything up to the last unit of a named one -- the device engine goes on behind them --, the third time the rest."""
    named = [i for i, u in enumerate(rest) if u.tid in (tids or ())]
    upto = len(rest) if refusals >= 3 else max(named) + 1 if named else 1
    return list(dict.fromkeys(u.tid for u in rest[:upto]))


class _Part:
    """What stage A hands to stage B: ``epoch`` of the cut it belongs to (_Replan), ``unit`` (None: a whole chromosome from
    the host engine), ``table`` (device engine: a callable that finishes it, or None for a slice without a record; the
    slot that holds its arrays is ``table._slot``), ``arrays`` (device engine: the CIGAR arrays on the device, else None)."""
    __slots__ = ("epoch", "unit", "table", "arrays")

    def __init__(self, epoch, unit, table, arrays):
        self.epoch, self.unit, self.table, self.arrays = epoch, unit, table, arrays


class _Replan:
    """Slices cut again with a larger margin: the hand-shake of stage A and stage B.  Who writes what:
      stage A   ``cut``: the epoch its current units were cut in; ``put``: parts queued in that epoch
      stage B   ``epoch``: what it accepts (parts of an older cut are dropped); ``acked``: (epoch, parts of it looked at); ``request``: (epoch, tid,
                coordinate, bases needed) of the slice it rejected; ``closed``: it has left its loop -- nothing will be acknowledged any more"""

    def __init__(self):
        self.cut, self.put = 0, 0
        self.epoch, self.acked, self.request, self.closed = 0, (0, 0), None, False

    def ack(self, epoch):                                      # stage B
        self.acked = (epoch, self.acked[1] + 1 if self.acked[0] == epoch else 1)

    def reject(self, epoch, tid, coord, needed):               # stage B
        self.request = (epoch, tid, coord, needed)
        self.epoch = epoch + 1

    def wanted(self):                                          # stage A: the request against its current cut, or None
        rp = self.request
        return rp if rp is not None and rp[0] == self.cut else None

    def all_acked(self):                                       # stage A
        return not self.put or self.acked == (self.cut, self.put)

    def recut(self):                                           # stage A
        self.cut, self.put = self.cut + 1, 0


class ChromosomeFeed:
    """See the module docstring.  ``chroms``: this rank's chromosomes in task order; ``references`` / ``lengths``: the
    BAM header's dictionary.  ``stats`` afterwards: seconds the feeder thread spent waiting for the decoder, uploading +
    scanning, and blocked on a full hand-over queue; bytes of packed CIGAR uploaded."""

    def __init__(self, bam_path, fasta, options, chroms, references, lengths, device="cuda", index=None, threads=0, depth=2,
                 engine=None, header_text="", tasks=None):
        self.bam_path, self.fasta, self.options = bam_path, fasta, options
        # tasks: {chromosome: [[start, end], ...]} -- the job's collection windows (cli.build_tasks).  With them the device engine
        # hands a chromosome over in SLICES of whole windows (ingest_gpu.DeviceDecoder.plan_units) instead of in one piece: the
        # first window of a 3 GB chromosome starts after its first ~200 MB, as the reference's window-by-window fetch does
        # (run_collection.py:23-26).  None: whole chromosomes.
        self.tasks = None if tasks is None else {c: [(int(a), int(b)) for a, b in w] for c, w in tasks.items()}
        self.header_text = header_text
        # where the BGZF blocks are inflated: "gpu" = on the device (ingest_gpu.DeviceDecoder), "cpu" = libdeflate on host
        # threads (io.bam.BamStream), "auto" (the default; SVX_INGEST overrides) = the device whenever it can: the file has a
        # .bai with its linear index.  On a 16-CPU GPU box the device engine takes 0.6 s for the 3.9 GB of the bench's 20-window
        # file, the host engine 1.15 s (DESIGN.md section 5 "Device-side ingestion"); a reference the device engine cannot take (a
        # linear index that does not match, a corrupt block) falls back to the host engine chromosome by chromosome.  Runs that
        # want the read bases (--hash / --graph) are served by the device engine too (svx_bam_walk_*_seq; the bases follow the
        # hand-over through the spill thread); which engine "auto" picks for them: AUTO_WITH_SEQ below.
        self.engine = engine or os.environ.get("SVX_INGEST", "auto")
        self.references, self.lengths = list(references), list(lengths)
        self.chroms = list(chroms)
        self.device, self.index, self.threads = device, index, threads
        self.with_seq = bool(options.hash or getattr(options, "graph", False))
        shm = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
        self.root = tempfile.mkdtemp(prefix="svx_feed_", dir=shm)
        self.slots = _SlotPool(self.root)
        self.decoded = queue.Queue(maxsize=2)                # stage A -> stage B: _Part, an exception, None at the end
        self.spill = queue.Queue()                           # stage B -> stage C: (table, the meta's event, sample), None at the end
        self.handover = queue.Queue(maxsize=depth)           # stage B -> owner thread
        self.samples = {}                                      # chrom -> [[lo, hi, key, Sample, meta], ...] (ascending; a whole chromosome: one entry) once the owner has seen them
        self.fresh = []                                        # (key, meta) not yet announced to the helpers
        self.error = None
        self.finished = False
        self.stats = {"engine": None, "decode_wait_s": 0.0, "upload_scan_s": 0.0, "handover_wait_s": 0.0, "cigar_bytes": 0, "records": 0,
                      "first_ready_s": None, "last_ready_s": None, "slices": 0, "replans": 0}
        self.replan = _Replan()
        self.decoder = None                                    # the device engine's DeviceDecoder, once stage A has built it
        self._want, self._covered = [], {}                     # stage B: tids not completely handed over yet, in task order; tid -> the coordinate up to which its windows have been
        self._scan_stream = None                               # stage B: the "scan" stream (a hardware queue of its own: svision_amd/streams.py)
        self._t0 = time.perf_counter()
        self._stop = False
        self.thread = threading.Thread(target=self._run, name="svx-feed", daemon=True)
        self.thread.start()

    def _mark(self, what):
        if self.decoder is not None:
            self.decoder._mark(what)

    # ---- stage B ---------------------------------------------------------------------------------------------------
    def _run(self):
        """Stage B, thread "svx-feed": starts stage A and stage C, then takes part after part from ``decoded`` (blocks on it 0.2 s at a
        time: ``decode_wait_s``) through _accept, _scan and _reject or _hand_over.  Whatever ends it, the owner gets its None (and ``error``)."""
        import torch
        try:
            tids = [self.references.index(c) for c in self.chroms]
            self._want = list(tids)
            if not torch.cuda.is_available():
                raise RuntimeError("ChromosomeFeed needs the GPU (svx_cigar_scan); there is no CPU fallback")
            engine = self.engine
            if engine == "auto":
                engine = AUTO_WITH_SEQ if self.with_seq else "gpu"
            if engine == "gpu" and (self.index is None or not str(self.device).startswith("cuda")):
                engine = "cpu"
            self.stats["engine"] = engine
            threading.Thread(target=self._decode, args=(engine, tids), name="svx-decode", daemon=True).start()
            self._scan_stream = streams.get("scan", self.device)
            threading.Thread(target=self._spill, name="svx-spill", daemon=True).start()
            while not self._stop:
                t0 = time.perf_counter()
                try:
                    part = self.decoded.get(timeout=0.2)
                except queue.Empty:
                    continue
                finally:
                    self.stats["decode_wait_s"] += time.perf_counter() - t0
                if part is None:
                    break
                if isinstance(part, BaseException):
                    raise part
                t0 = time.perf_counter()
                span = self._accept(part)
                if span is None:
                    continue
                if not self._want:
                    break
                sample = None if part.table is None else self._scan(part)
                if sample is not None and part.unit is not None and not self._slice_complete(part.unit, sample):
                    self._reject(part, sample, *span[:2])
                else:
                    self._hand_over(part, sample, t0, *span)
            while self._want and not self._stop:
                t_ = self._want.pop(0)
                self._emit_empty(t_, self._covered.get(t_, 0))
            if self.decoder is not None:
                self.stats["device_decoder"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in self.decoder.stats.items()}
                self.stats["device_decoder"]["trace"] = ["%.3f %s" % (t + (self.decoder._t0 - self._t0), w) for t, w in self.decoder.trace[:400]]
        except BaseException as exc:                           # noqa: BLE001 -- surfaces in the owner thread (poll / get)
            self.error = exc
            self._stop = True
            try:
                while True:                                    # let stage A run into its stop flag
                    self.decoded.get_nowait()
            except queue.Empty:
                pass
        finally:
            self.replan.closed = True                          # stage A's _settle() / _queue() must not wait for acknowledgements that cannot come
            self.spill.put(None)
            self.handover.put(None)

    def _accept(self, part):
        """Stage B; host work, may block on a full ``handover`` (_emit_empty).  A part of a cut that has been replaced -> None.  Else the
        table is finished (device engine: the QNAME ids), the chromosomes in front of it without a record in the file (or in the rest of it) are
        handed over empty, and -> (tid, lo, hi, last): the windows [lo, hi) the part serves -- a whole chromosome: all not handed over yet."""
        if part.epoch != self.replan.epoch:                    # decoded before the slices were cut again (a margin that was too small)
            return None
        self._mark("consumer: got a part")
        if self.decoder is not None and os.environ.get("SVX_TIMING"):
            from . import sample as _sample_mod
            _sample_mod._MARK = self.decoder._mark
        if callable(part.table):
            part.table = part.table()
        unit = part.unit
        tid = unit.tid if unit is not None else int(part.table.tid[0])
        while self._want and self._want[0] != tid:
            t_ = self._want.pop(0)
            self._emit_empty(t_, self._covered.get(t_, 0))
        lo = self._covered.get(tid, 0) if unit is None else max(unit.lo, self._covered.get(tid, 0))
        last = unit is None or unit.last
        return tid, lo, float("inf") if last else unit.hi, last

    def _scan(self, part):
        """Stage B, on the "scan" stream: upload (host engine) + svx_cigar_scan -> the part's Sample.  Blocks on the device (the read-back)."""
        import torch
        with torch.cuda.stream(self._scan_stream):
            if part.arrays is None:
                sample = Sample.from_table(part.table, self.fasta, self.options.min_sv_size, self.device)
            else:
                sample = Sample.from_device(part.table, self.fasta, self.options.min_sv_size, *part.arrays)
        self._mark("consumer: scanned")
        return sample

    def _reject(self, part, sample, tid, lo):
        """Stage B; blocks on nothing.  The records of this slice reach farther than the margin it was cut with: it may miss records its
        windows' clusters count or genotype with.  Nothing of it is handed over; stage A cuts the rest of the file again (_Replan)."""
        needed = self._slice_needs(part.unit, sample)
        self.stats["replans"] += 1
        self._mark("slice %r rejected: its windows need %d bases beyond them" % (part.unit, needed))
        self.replan.reject(part.epoch, tid, lo, needed)
        sample.device_buffers = None
        self.slots.give(part.table._slot.dir)

    def _hand_over(self, part, sample, t0, tid, lo, hi, last):
        """Stage B; blocks on a full ``handover``.  The scan's arrays into the slot, the meta, the spill job (device engine) -- or, a slice
        without a record, its windows empty --, then the one acknowledgement stage A waits for."""
        table = part.table
        if table is None:
            self._emit_empty(tid, lo, hi)
        else:
            meta = part_meta(table._slot, table, sample, self.references, self.lengths, self.options.min_sv_size, self.with_seq)
            self.stats["upload_scan_s"] += time.perf_counter() - t0
            self.stats["cigar_bytes"] += int(table.cigar.nbytes)
            self.stats["records"] += len(table)
            self.stats["slices"] += 1
            if part.arrays is not None:                        # device engine: the host copy of the CIGAR words follows later
                meta["lazy_cigar"] = int(table.cigar.size)
                meta["spilled"] = threading.Event()
                table.cigar.event = meta["spilled"]            # (LazyCigar: a reader in THIS process waits for the spill)
                if table.seq_packed is not None:               # (LazySeq: the bases follow the same way, behind the words)
                    meta["lazy_seq"] = int(table.seq_packed.size)
                    table.seq_packed.event = meta["spilled"]
                self.spill.put((table, meta["spilled"], sample))
            else:
                # host engine: the upload served the scan and nothing else (windows of a file-driven run are never scanned
                # again: their chromosome's Sample is final) -- the slice's device arrays go back to the allocator now, not when
                # the whole chromosome has been voted (a chromosome's slices held their buffers until release())
                sample.device_buffers = None
            self._mark("handed over %s [%s, %s) (scan + slot writes)" % (self.references[tid], lo, hi))
            self._put((self.references[tid], lo, hi, sample, meta))
        self._covered[tid] = hi
        if last:
            self._want.pop(0)
        self.replan.ack(part.epoch)

    @staticmethod
    def _window_needs(unit, table):
        """Per window [a, b) of the slice: (a, b, lo, hi), the reach [lo, hi) it needs records of.  A window collects on the records that overlap
        it; the coordinates of their signatures -- and so the extents of the clusters the window reports -- stay within those records'
        [pos - read length, end + read length] (inserted / re-placed pieces), the cluster coverage (classes.py:165-170) counts the records
        overlapping those extents and the genotyper looks 1000 bases farther (genotype.py:22-26).  So the window needs every record
        overlapping [min(pos - l_seq) - 1000, max(end + l_seq) + 1000) of ITS records."""
        tid, ref_end = int(table.tid[0]), table.ref_end()
        for a, b in unit.windows:
            rows = table.fetch(tid, a, b)
            lo, hi = a, b
            if rows.size:
                l_seq = table.l_seq[rows].astype(np.int64)
                lo, hi = min(a, int((table.pos[rows].astype(np.int64) - l_seq).min())), max(b, int((ref_end[rows] + l_seq).max()))
            yield a, b, lo - 1000, hi + 1000

    @staticmethod
    def _slice_complete(unit, sample):
        """Does the slice hold every record its windows can touch (_window_needs)?  On the left the slice starts at the
        linear-index entry of ``left_edge`` (every record reaching beyond that coordinate lies behind it), on the right it ends
        in front of a record that starts at or behind its last one (the file is sorted)."""
        table = sample.table
        if len(table) == 0:
            return unit.left_edge is None and unit.to_end
        return not any((unit.left_edge is not None and unit.left_edge > lo) or (not unit.to_end and int(table.pos[-1]) < hi)
                       for _a, _b, lo, hi in ChromosomeFeed._window_needs(unit, table))

    @staticmethod
    def _slice_needs(unit, sample):
        """The margin (bases beyond its windows) the slice turned out to need: what it is cut again with, doubled (grow_margin)."""
        if len(sample.table) == 0:
            return 0
        return max((max(a - lo, hi - b) for a, b, lo, hi in ChromosomeFeed._window_needs(unit, sample.table)), default=1000)

    # ---- stage C ---------------------------------------------------------------------------------------------------
    def _spill(self):
        """Stage C, thread "svx-spill", on the "spill" stream: host copies of the device-decoded CIGAR words (ingest_gpu.spill_cigar) and,
        with_seq, of the bases (ingest_gpu.spill_seq), after the hand-over.  Blocks on ``spill`` and on the device (the copies)."""
        import torch
        from .ingest_gpu import spill_cigar, spill_seq
        stream = streams.get("spill", self.device)
        for table, done, sample in iter(self.spill.get, None):
            try:
                with torch.cuda.stream(stream):
                    spill_cigar(table)
                    if getattr(table, "_d_seq", None) is not None:
                        table._d_seq.record_stream(stream)
                        spill_seq(table)
                    if sample.device_buffers is not None:      # (the arrays were last used on this stream: the spill's copy)
                        for t in sample.device_buffers[:3]:
                            t.record_stream(stream)
                table._d_cigar = table._d_seq = None
                sample.device_buffers = None                   # the device arrays of the slice: scanned, spilled, never read again
            except BaseException as exc:                       # noqa: BLE001 -- a helper that needs the words would wait for ever
                self.error = self.error or exc
            finally:
                done.set()

    # ---- stage A ---------------------------------------------------------------------------------------------------
    def _decode(self, engine, tids):
        """Stage A, thread "svx-decode": the rank's chromosomes as _Parts into ``decoded``, then None -- or the exception
        that ended it.  Blocks on a full ``decoded`` and, device engine, on the decoder's pipeline and in _settle."""
        try:
            (self._decode_device if engine == "gpu" else self._host_parts)(tids)
            self._queue(None)
        except BaseException as exc:                           # noqa: BLE001
            self._queue(exc)

    def _queue(self, item):
        """Stage A: ``item`` into ``decoded`` -> True; False once the feed is closing or stage B has gone."""
        while not self._stop and not self.replan.closed:
            try:
                self.decoded.put(item, timeout=0.2)
            except queue.Full:
                continue
            self.replan.put += isinstance(item, _Part)
            return True
        return False

    def _host_parts(self, which):
        """Stage A, host engine: BGZF inflate on host threads (libdeflate, io.bam.BamStream) -- whole chromosomes, each
        decoded into this process's memory and written to a slot from there.  -> False: the feed is closing."""
        logging.info("%s: records decoded by the host engine%s", self.bam_path, "" if self.index is None else " through %s" % self.index)
        stream = BamStream(self.bam_path, with_seq=self.with_seq, threads=self.threads, tids=which, index=self.index)
        try:
            for table in stream:
                table._slot = self.slots.take()
                put_table(table._slot, table, self.with_seq)
                if not self._queue(_Part(self.replan.cut, None, table, None)):
                    return False
        finally:
            stream.close()
        return True

    def _windows_of(self, tid):
        return self.tasks.get(self.references[tid])

    def _decode_device(self, tids):
        """Stage A, device engine: BGZF inflate + record packing on the device, pass after pass over the units left --
        a pass ends with the units, with stage B's request to cut them again, or with a refusal (host_takes)."""
        from .ingest_gpu import DeviceDecoder
        # pread threads of the device engine: copies out of the page cache, ~2 GB/s each (SVX_READ_THREADS overrides)
        n_read = int(os.environ.get("SVX_READ_THREADS", "0")) or min(8, max(1, self.threads))
        dec = self.decoder = DeviceDecoder(self.bam_path, self.index, self.references, self.lengths, self.header_text, self.device,
                                           threads=n_read, take_slot=self.slots.take, with_seq=self.with_seq)
        why = dec.unusable(tids)
        if why is not None:
            logging.info("%s: %s", self.index, why)
            self.stats["engine"] = "cpu"
            return self._host_parts(tids)
        logging.info("%s: records decoded by the device engine through %s", self.bam_path, self.index)
        windows_of = self._windows_of if self.tasks is not None and not getattr(self.options, "contig", False) else None
        # (SVX_SLICE_MARGIN: tests -- a margin that is too small must be noticed and the slices cut again)
        margin = (int(os.environ.get("SVX_SLICE_MARGIN", "0")) or dec.estimate_reach(tids)) if windows_of is not None else 0
        units = dec.plan_units(tids, windows_of, margin)
        refusals = 0
        while units and not self._stop:
            done, exc = self._device_pass(dec, units)
            if done is None:
                return
            request = self._settle()                           # (an error behind a rejected slice: cut again first, the error will come back)
            if request is not None:
                # a slice's records reach farther than the margin guessed from the file's first reads (ONT: a log-normal
                # tail): everything from that slice on is cut again with twice what it needed
                _epoch, tid, coord, needed = request
                margin = grow_margin(needed, margin)
                self.replan.recut()
                logging.info("device ingestion: slices of %s cut again from %d on with a margin of %d bases", self.references[tid], coord, margin)
                units = dec.plan_units(tids, windows_of, margin, resume=(tid, coord))
            elif exc is None:
                break
            else:
                refusals += 1
                rest = units[done:]
                bad = host_takes(rest, exc.tids, refusals)
                blamed = len({u.tid for u in rest} & set(exc.tids or ()))
                logging.warning("device ingestion failed at reference %s (%s): decoding %s on the host",
                                ", ".join(self.references[t] for t in bad[-max(1, blamed):]), exc,
                                "the rest of the file" if refusals >= 3 else "%d reference(s)" % len(bad))
                if not self._host_parts(bad):
                    return
                units = [u for u in rest if u.tid not in bad]
        self._settle()

    def _device_pass(self, dec, units):
        """Stage A: one run of the decoder's pipeline over ``units`` -> (parts queued, the DeviceIngestError that ended it
        or None); it also ends when stage B asks for another cut.  (None, None): the feed is closing."""
        from .ingest_gpu import DeviceIngestError
        done = 0
        try:
            for unit, finish, arrays in dec.units_pipelined(units):
                if self.replan.wanted() is not None:
                    break
                if not self._queue(_Part(self.replan.cut, unit, finish, arrays)):
                    return None, None
                done += 1
        except DeviceIngestError as exc:
            return done, exc
        return done, None

    def _settle(self):
        """Stage A: wait until stage B has looked at everything queued in this cut (the LAST slice may be the one it rejects) -> its request or None."""
        while not self._stop and not self.replan.closed and self.replan.wanted() is None and not self.replan.all_acked():
            time.sleep(0.0005)
        return self.replan.wanted()

    def _emit_empty(self, tid, lo=0, hi=float("inf")):
        """Windows [lo, hi) of a chromosome without records there: they still exist as tasks (SVision:172-201) and yield nothing."""
        meta = {"dir": None, "references": self.references, "lengths": self.lengths, "min_sv": self.options.min_sv_size, "n": 0,
                "with_seq": self.with_seq, "header_text": ""}
        self._put((self.references[tid], lo, hi, empty_sample(self.references, self.lengths, self.fasta, self.options.min_sv_size), meta))

    def _put(self, item):
        t0 = time.perf_counter()
        self.handover.put(item)
        self.stats["handover_wait_s"] += time.perf_counter() - t0

    # ---- last: the owner thread ------------------------------------------------------------------------------------
    def poll(self, block=False):
        """Move the chromosomes / slices the feeder has finished into ``samples`` (and onto the ``fresh`` list of what the
        helpers have not been told yet); ``block``: wait until at least one arrives or the stream ends.  -> whether any arrived."""
        got = False
        while not self.finished:
            try:
                item = self.handover.get(block=block and not got, timeout=0.25 if block and not got else None)
            except queue.Empty:
                if block and not got:
                    continue
                break
            if item is None:
                self.finished = True
                if self.error is not None:
                    raise self.error
                break
            chrom, lo, hi, sample, meta = item
            key = next(_KEYS)                                  # unique in the process: a helper may still hold a key of an earlier feed
            now = time.perf_counter() - self._t0
            if self.stats["first_ready_s"] is None:
                self.stats["first_ready_s"] = now
            self.stats["last_ready_s"] = now
            self.samples.setdefault(chrom, []).append([lo, hi, key, sample, meta])
            self.fresh.append((key, chrom, meta))
            got = True
        return got

    def _find(self, chrom, start):
        for ent in self.samples.get(chrom, ()):
            if start is None or ent[0] <= start < ent[1]:
                return ent
        return None

    def get(self, chrom, block=True, start=None):
        """-> (key, Sample) of the part of a chromosome that serves the collection window starting at ``start`` (None: its
        first part -- a whole chromosome is one part), or (None, None) when it is not ready and ``block`` is False."""
        while True:
            ent = self._find(chrom, start)
            if ent is not None:
                return ent[2], ent[3]
            if self.finished:
                raise KeyError("chromosome %s%s is not part of this feed" % (chrom, "" if start is None else " at %s" % start))
            self.poll(block=block)
            if not block and self._find(chrom, start) is None:
                return None, None

    def keys_of(self, chrom):
        return [ent[2] for ent in self.samples[chrom]]

    def take_fresh(self):
        """(key, chrom, meta) of the parts that arrived since the last call: what the helpers must be sent."""
        out, self.fresh = self.fresh, []
        # (the meta of a chromosome goes through a pipe: without the owner-side event)
        return [(k, c, None if m is None else {a: b for a, b in m.items() if a != "spilled"}) for k, c, m in out]

    def release(self, chrom):
        """The chromosome is done (its windows voted and stitched): free its device buffers and shared memory."""
        for ent in self.samples.get(chrom, ()):
            _lo, _hi, _key, sample, meta = ent
            if sample is None:
                continue
            sample.device_buffers = None
            ent[3], ent[4] = None, None
            if meta is not None and meta["dir"] is not None:
                if meta.get("spilled") is not None:
                    meta["spilled"].wait(timeout=120)          # the slot must not be reused under a running spill
                self.slots.give(meta["dir"])

    def close(self):
        self._stop = True
        try:
            while self.thread.is_alive():
                try:
                    self.handover.get_nowait()
                except queue.Empty:
                    time.sleep(0.005)
        finally:
            shutil.rmtree(self.root, ignore_errors=True)


def load_shared_sample(meta, fasta):
    """Helper-process side: the chromosome a ChromosomeFeed announced, mapped from shared memory (copy-on-write)."""
    d = meta["dir"]
    if d is None:
        return empty_sample(meta["references"], meta["lengths"], fasta, meta["min_sv"], meta["header_text"])
    arrays = meta["arrays"]

    def arr(name, dtype):
        if name not in arrays or arrays[name][1] == 0:
            return np.empty(0, dtype)
        return np.memmap(os.path.join(d, name + ".bin"), dtype=np.dtype(dtype), mode="c", shape=(arrays[name][1],))
    t = {name: arr(name, dtype) for name, dtype in TABLE_ARRAYS + (SEQ_ARRAYS if meta["with_seq"] else ())}
    names = bytes(t["names"]).decode().split("\n")[:-1] if t["names"].size else []
    cig_off = t["cig_off"] if t["cig_off"].size else np.zeros(1, np.int64)
    table = AlignmentTable(meta["references"], meta["lengths"], t["tid"], t["pos"], t["flag"], t["mapq"], t["l_seq"], t["name_id"], names,
                           t["cigar"], cig_off, meta["header_text"], t.get("seq_packed"), t.get("seq_off"))
    if meta.get("lazy_cigar") is not None:                     # device engine: the words arrive in the slot a little later
        from .ingest_gpu import LazyCigar
        table.cigar = LazyCigar(meta["lazy_cigar"], os.path.join(d, "cigar.bin"), os.path.join(d, "cigar.ready"))
    if meta.get("lazy_seq") is not None:                       # ... and, with_seq, the bases behind them
        from .ingest_gpu import LazySeq
        table.seq_packed = LazySeq(meta["lazy_seq"], os.path.join(d, "seq_packed.bin"), os.path.join(d, "seq.ready"))
    from . import kernels
    gaps, gap_off, stats = (arr(name, dtype) for name, dtype in zip(SCAN_ARRAYS, (kernels.GAP_DTYPE, np.int64, np.int32)))
    return Sample.with_scan(table, fasta, meta["min_sv"], (gaps, gap_off, np.asarray(stats).reshape(meta["stats_shape"])))
