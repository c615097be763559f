"""The ``SVision`` command line on MI355X: same arguments, same outputs.

Mirror of the reference driver (``SVision``): argument surface :27-106,
input checks :141-157, window tasking :164-234 (including the ``-c chr:a-b`` quirk that
windows restart at 0), Step 1 collection :259-294, Step 2 prediction :296-328, score range +
merge :331-339, cleanup :370-372.  The two process pools are replaced by one process per
GPU (chromosomes sharded across ranks when launched under torchrun, see dist.py).

``run`` is its steps in order: input -> plan -> (device set-up) -> compute -> exchange -> merge, inside the run's log.
"""
import argparse
import collections
import contextlib
import datetime
import logging
import os
import shutil
import sys
from time import localtime, strftime

import numpy as np

from . import __version__, dist as sdist
from .io.bam import Fasta, read_bam

REFERENCE_VERSION = "1.4"      # ##source line of the VCF the reference writes (src/version.py)


def parse_arguments(arguments=None):
    p = argparse.ArgumentParser(formatter_class=argparse.RawDescriptionHelpFormatter,
                                description="SVision (MI355X hot path %s)\n\nShort Usage: SVision [parameters] -o <output path> "
                                            "-b <input bam path> -g <reference> -m <model path>" % __version__)
    g = p.add_argument_group("Input/Output parameters")
    g.add_argument("-o", dest="out_path", type=os.path.abspath, required=True, help="Absolute path to output")
    g.add_argument("-b", dest="bam_path", type=_bam_arg, required=True, help="Absolute path to bam file; SVX_DEVICE_SORT=write or =1: ``-`` is "
                   "an aligner's output on standard input -- SAM text; a BAM there (dorado aligner, pbmm2) is copied into a file first under "
                   "=write and refused under =1, unless SVX_PIPE_BAM=stream takes it in one pass")
    g.add_argument("-m", dest="model_path", type=os.path.abspath, required=True, help="Absolute path to CNN predict model")
    g.add_argument("-g", dest="genome", type=os.path.abspath, required=True, help="Absolute path to your reference genome")
    g.add_argument("-n", dest="sample", type=str, required=True, help="Name of the BAM sample name")
    g = p.add_argument_group("Optional parameters")
    g.add_argument("-t", dest="thread_num", type=int, default=1, help="Thread numbers (default: %(default)s)")
    g.add_argument("-s", dest="min_support", type=int, default=5, help="Minimum support read number required for SV calling (default: %(default)s)")
    g.add_argument("-c", dest="chrom", type=str, default=None, help="Specific region (chr1:xxx-xxx) or chromosome (chr1) to detect")
    g.add_argument("--hash", action="store_true", default=False, help="Activate local realignment for unmapped sequences (default: %(default)s)")
    g.add_argument("--qname", action="store_true", default=False, help="Report support names for each events (default: %(default)s)")
    g.add_argument("--graph", action="store_true", default=False, help="Report graph for events (default: %(default)s)")
    g.add_argument("--contig", action="store_true", default=False, help="Activate contig mode (default: %(default)s)")
    g.add_argument("--debug", action="store_true", default=False, help="Activate debug mode and keep intermedia outputs (default: %(default)s)")
    g = p.add_argument_group("Collect parameters")
    g.add_argument("--min_mapq", type=int, default=10, help="Minimum mapping quality of reads to consider (default: %(default)s)")
    g.add_argument("--min_sv_size", type=int, default=50, help="Minimum SV size to detect (default: %(default)s)")
    g.add_argument("--max_sv_size", type=int, default=1000000, help="Maximum SV size to detect (default: %(default)s)")
    g.add_argument("--window_size", type=int, default=10000000, help="The sliding window size in segment collection (default: %(default)s)")
    g = p.add_argument_group("Cluster parameters")
    g.add_argument("--patition_max_distance", type=int, default=5000, help="Maximum distance to partition signatures (default: %(default)s)")
    g.add_argument("--cluster_max_distance", type=float, default=0.3, help="Clustering maximum distance for a partition (default: %(default)s)")
    g = p.add_argument_group("Predict parameters")
    g.add_argument("--batch_size", type=int, default=128, help="Batch size for the CNN prediction model (default: %(default)s)")
    g = p.add_argument_group("Genotype parameters")
    g.add_argument("--min_gt_depth", type=int, default=4, help="Minimum reads required for genotyping (default: %(default)s)")
    g.add_argument("--homo_thresh", type=float, default=0.8, help="Minimum variant allele frequency to be called as homozygous (default: %(default)s)")
    g.add_argument("--hete_thresh", type=float, default=0.2, help="Minimum variant allele frequency to be called as heterozygous (default: %(default)s)")
    g = p.add_argument_group("Hash table parameters")
    g.add_argument("--k_size", type=int, default=10, help="Size of kmer (default: %(default)s)")
    g.add_argument("--min_accept", type=int, default=50, help="Minimum match length for realignment (default: %(default)s)")
    g.add_argument("--max_hash_len", type=int, default=1000, help="Maximum length of unmapped sequence length for realignment (default: %(default)s)")
    return p.parse_args(sys.argv[1:] if arguments is None else arguments)


def build_tasks(options, references, lengths, fasta_refs):
    """{chrom: [[start, end], ...]} in BAM-header order (SVision:164-234)."""
    length_of = dict(zip(references, lengths))
    window = options.window_size
    tasks = {}
    if options.chrom is None:
        for chrom in references:
            n = length_of[chrom]
            if chrom not in fasta_refs:
                continue
            if options.contig:
                window = n
            if n < window:
                tasks.setdefault(chrom, []).append([0, n])
                continue
            pos = 0
            for _ in range(int(n / window)):
                tasks.setdefault(chrom, []).append([pos, pos + window])
                pos += window
            if pos < n:
                tasks.setdefault(chrom, []).append([pos, n])
        return tasks
    chrom = options.chrom
    if chrom in fasta_refs:
        start, end = 0, length_of[chrom]
    else:
        cords = chrom.split(":")[1]
        chrom, start, end = chrom.split(":")[0], int(cords.split("-")[0]), int(cords.split("-")[1])
    tasks[chrom] = []
    region_length = end - start + 1
    if region_length < window:
        tasks[chrom].append([start, end])
    else:
        pos = 0                                           # upstream restarts at 0, not at `start`
        for _ in range(int(region_length / window)):
            tasks[chrom].append([pos, pos + window])
            pos += window
        if pos < region_length:
            tasks[chrom].append([pos, region_length])
    return tasks


class RunDirs:
    """Where a run writes: the output directory, its three working directories and the names of the files in them.  The file names
    carry ``options.min_support``, read when a name is asked for (``--contig`` changes it once the run has begun)."""

    def __init__(self, options, segments=None, predict_results=None):
        self.options, self.out_path = options, options.out_path
        self.segments = segments or os.path.join(self.out_path, "segments")
        self.predict_results = predict_results or os.path.join(self.out_path, "predict_results")
        self.graphs = os.path.join(self.out_path, "graphs")

    def part_bed(self, chrom, part):
        """The segment signatures of window ``part`` of ``chrom``."""
        return os.path.join(self.segments, "%s.segments.%d.bed" % (chrom, part))

    def all_bed(self, chrom):
        """The part beds of ``chrom`` in window order (upstream: ``cat``)."""
        return os.path.join(self.segments, chrom + ".segments.all.bed")

    def predict_prefix(self, chrom):
        """What Predict.run is given: it writes ``<prefix>.vcf`` and ``<prefix>.score.txt``."""
        return os.path.join(self.predict_results, "%s.predict.s%s" % (chrom, self.options.min_support))

    def predict_vcf(self, chrom):
        return self.predict_prefix(chrom) + ".vcf"

    def score_txt(self, chrom):
        return self.predict_prefix(chrom) + ".score.txt"

    def merged_vcf(self, graph=False):
        """The run's result; ``graph``: the form Step 3 leaves in its place."""
        return os.path.join(self.out_path, "%s.svision.s%s%s.vcf" % (self.options.sample, self.options.min_support, ".graph" if graph else ""))


class _Ticker:
    """SVX_TIMING=1: wall time of the phases of a run on stdout."""

    def __init__(self):
        import time
        self.clock, self.last, self.on = time.time, time.time(), bool(os.environ.get("SVX_TIMING"))

    def lap(self):
        """Seconds since the last lap or phase line; prints nothing."""
        now = self.clock()
        spent, self.last = now - self.last, now
        return spent

    def __call__(self, what):
        spent = self.lap()
        if self.on:
            print("%-36s %.3f s" % (what, spent), flush=True)


@contextlib.contextmanager
def _run_log(work_dir, rank, ws):
    """The run's own log file on the root logger, for as long as the run lasts: the handler is removed and closed whichever way
    the block is left (an exit, an exception), so that the next run in this process writes to its own file only."""
    root = logging.getLogger()
    root.setLevel(logging.INFO)
    fh = logging.FileHandler("%s/SVision_%s%s.log" % (work_dir, strftime("%y%m%d_%H%M%S", localtime()), "" if ws == 1 else ".rank%d" % rank), mode="w")
    fh.setFormatter(logging.Formatter("%(asctime)s [%(levelname)-7.7s]  %(message)s"))
    root.addHandler(fh)
    try:
        yield
    finally:
        root.removeHandler(fh)
        fh.close()


def _rank_shard(chroms, references, lengths, rank, ws):
    """The chromosomes of ``chroms`` that rank ``rank`` of ``ws`` works on: shared out by length, longest first (dist.shard_chromosomes)."""
    length_of = dict(zip(references, lengths))
    return sdist.shard_chromosomes(chroms, [length_of.get(c, 1) for c in chroms], ws)[rank]


def load_rank_table(options, rank, ws):
    """The alignment records rank ``rank`` of ``ws`` needs.  With a ``.bai`` next to the BAM and more than one rank, a
    rank is a set of chromosomes: the header gives the task list, the index gives the byte range holding this rank's
    records, and only that range is read and inflated (upstream: AlignmentFile.fetch(chrom), run_collection.py:26)."""
    from .io.bam import find_index
    index = find_index(options.bam_path)                        # (.bai, else .csi)
    if ws == 1 or index is None:
        return read_bam(options.bam_path, with_seq=bool(options.hash or options.graph))
    head = read_bam(options.bam_path, tids=[], index=index)
    tasks = build_tasks(options, head.references, head.lengths, Fasta(options.genome).references)
    shard = _rank_shard(list(tasks), head.references, head.lengths, rank, ws)
    table = read_bam(options.bam_path, with_seq=bool(options.hash or options.graph), tids=[head.references.index(c) for c in shard], index=index)
    logging.info("rank %d/%d: %d records of %s decoded through %s", rank, ws, len(table), ",".join(shard) or "-", index)
    return table


def _load_unsorted(options, several=None):
    """SVX_DEVICE_SORT=1 and a header that does not say ``SO:coordinate``, an aligner's SAM text, ``-b -`` or a list of inputs
    (``several``): everything taken apart and the records sorted on the device (svision_amd/ingest_sort.py) -> the resident Sample the
    run goes on with.  No alignment file is written.  load_sample reads ``SVX_PIPE_BAM`` itself: "stream" takes a BAM on a pipe."""
    import time
    import torch
    from .ingest_sort import SortIngestError, load_sample
    t0 = time.perf_counter()
    if torch.cuda.is_available():
        torch.cuda.set_device(sdist.local_device_index())
    stats = {}
    try:
        sample = load_sample(several or options.bam_path, Fasta(options.genome), options.min_sv_size,
                             device=torch.device("cuda", torch.cuda.current_device()), with_seq=bool(options.hash or options.graph), stats=stats)
    except SortIngestError as exc:
        logging.error("%s", exc)
        raise SystemExit(1)
    kinds = stats.get("inputs", ["bam"])
    logging.info("%s is %s: %d records sorted on the device in %.2f s (%d range(s), %d radix passes)", options.bam_path,
                 "%d inputs" % len(kinds) if len(kinds) > 1 else "not coordinate sorted" if kinds[0] == "bam" else "a BAM on a pipe" if kinds[0] == "bam_pipe" else "SAM text",
                 stats["records"], time.perf_counter() - t0, stats["ranges"], stats["passes"])
    return sample


def _write_sorted(options):
    """SVX_DEVICE_SORT=write and a header that does not say ``SO:coordinate``, or an aligner's SAM text: the coordinate-sorted BAM and its .bai written into the
    output directory (svision_amd/sort.py) -> the sorted file's path, which stays there.  The sort runs in a process of its own: this
    one has not touched the device when the helpers of ``-t N`` are forked.  It inherits the environment: ``SVX_SORT_TABLES=dynamic``
    there is ``--tables dynamic`` (Huffman codes built per block; default: the fixed code), ``SVX_SORT_MEMORY=BYTES`` (K, M or G) is
    ``--memory``: the device memory for the records' inflated bytes, beyond which the file is written in spans, a pass over the input
    for each (default: half of the free device memory), ``SVX_SORT_INDEX=csi`` is ``--csi``: the index written as a ``.csi``, the format for
    positions from 2^29 on, ``SVX_SORT_RETAG=1`` is ``--retag``: colliding @RG / @PG IDs of several inputs renamed and their records' tags
    rewritten, ``SVX_SORT_DROP_TAGS=fi,fp,ri,rp`` / ``SVX_SORT_KEEP_TAGS=RG,NM`` are ``--drop-tags`` / ``--keep-tags``: optional fields
    removed from every record of the sorted file (BAM inputs only; the caller reads none of them).  ``-b a.bam,b.bam,c.sam`` (:func:`_input_list`): the inputs merged into the one sorted
    file ``OUT/<first input's stem>.merged.sorted.bam``."""
    import json
    import subprocess
    import sys
    import time
    t0 = time.perf_counter()
    inputs = _input_list(options.bam_path) or [options.bam_path]       # several: merged into OUT/<first input's stem>.merged.sorted.bam
    name = "stdin" if inputs[0] == "-" else os.path.basename(inputs[0])
    out = os.path.join(options.out_path, (name[:-4] if name.endswith((".bam", ".sam")) else name) + (".merged" if len(inputs) > 1 else "") + ".sorted.bam")
    stats_path = out + ".stats.json"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, "-m", "svision_amd.sort"] + inputs + ["-o", out, "--stats-json", stats_path,
                        "--device", "cuda:%d" % int(os.environ.get("LOCAL_RANK", "0"))], capture_output=True, text=True, env=env)      # (``-``: the child inherits standard input)
    try:
        if r.stderr.strip():                                        # the child's whole stderr (a traceback with its context) for the log
            logging.debug("svision_amd.sort (exit status %d) wrote:\n%s", r.returncode, r.stderr.rstrip())
        if r.returncode != 0:
            logging.error("%s", (r.stderr.strip().splitlines() or ["svision_amd.sort failed"])[-1])
            raise SystemExit(1)
        with open(stats_path) as f:
            stats = json.load(f)
    finally:
        if os.path.exists(stats_path):
            os.unlink(stats_path)
    logging.info("%s is %s: %d records sorted on the device in %.2f s (%d range(s), %d radix passes)", options.bam_path,
                 "%d inputs to merge" % len(inputs) if len(inputs) > 1 else "SAM text" if stats.get("input") == "sam" else "not coordinate sorted", stats["records"], time.perf_counter() - t0,
                 stats["ranges"], stats["passes"])
    logging.info("sorted file: %s (+ its index), %d BGZF blocks, %d -> %d bytes, written in %d span(s) under a budget of %d bytes for the records "
                 "(SVX_SORT_MEMORY)", out, stats["blocks"], stats["inflated_bytes"], stats["compressed_bytes"], stats["spans"], stats["memory_bytes"])
    return out


# What a run reads.  ``sample``: the resident Sample (handed in, or sorted on the device), None when the file is streamed chromosome by
# chromosome; ``index`` / ``build_index``: the streamed file's .bai, or that it is to be built on the device (both unset for a Sample).
RunInput = collections.namedtuple("RunInput", "sample fasta references lengths index build_index")


def _bam_arg(value):
    """``-b``: an absolute path; ``-`` -- standard input, alone or as a part of a comma list -- stays as it is."""
    return value if value == "-" or "-" in value.split(",") else os.path.abspath(value)


def _input_list(bam_path):
    """A ``-b`` value that names no existing file, but whose comma-separated parts all do -> those files (absolute paths); else None.
    One part may be ``-``, standard input."""
    if bam_path == "-" or os.path.exists(bam_path) or "," not in bam_path:
        return None
    parts = [p if p == "-" else os.path.abspath(p) for p in bam_path.split(",")]
    return parts if parts.count("-") <= 1 and all(p == "-" or os.path.isfile(p) for p in parts) else None


def _is_stream(path):
    from . import sort
    return sort.is_stream(path)


def _is_sam_text(path):
    from .io import sam
    try:
        with open(path, "rb") as f:
            return sam.is_sam_text(f.read(1 << 20))
    except OSError:
        return False


def _open_input(options, sample, ws, tick):
    """Input step.  Needs the options, the caller's Sample or None, and the world size; touches no device and no process group unless
    an unsorted file is sorted (one rank, before any fork).  -> RunInput.  Refuses with SystemExit(1): a file that is not coordinate
    sorted without SVX_DEVICE_SORT=1 / =write, and SVX_DEVICE_SORT=1 / =write or SVX_BUILD_INDEX=1 (with no .bai) in a run of several
    ranks.  SVX_DEVICE_SORT=write: the sorted file is written into the output directory by a child process, ``options.bam_path`` is set to
    it, and the step answers as for any sorted, indexed file."""
    from . import sample as _sample
    from .io.bam import find_index, read_bam_header
    if sample is None:
        # file-driven run: header now, the records chromosome by chromosome while the pipeline runs (ingest.ChromosomeFeed)
        several = _input_list(options.bam_path)
        # (a path that is no regular file -- a FIFO, /dev/fd/N -- is a pipe like ``-``: it is seen once, so no byte of it is read here)
        piped = options.bam_path == "-" or bool(several and "-" in several) or (several is None and _is_stream(options.bam_path))
        switch = os.environ.get("SVX_DEVICE_SORT")
        if piped and switch not in ("write", "1"):
            logging.error("-b %s: standard input or a pipe is taken under SVX_DEVICE_SORT=write, which sorts an aligner's output on the device in one "
                          "pass and writes the sorted BAM, and under SVX_DEVICE_SORT=1, which calls from it and writes no alignment file",
                          "-" if several or options.bam_path == "-" else options.bam_path)
            raise SystemExit(1)
        if several and switch not in ("write", "1"):
            logging.error("-b names %d files: SVX_DEVICE_SORT=write merges them into one sorted BAM on the device, SVX_DEVICE_SORT=1 calls from "
                          "them as they are (one rank); every other setting takes one file -- merge them first with "
                          "`python -m svision_amd.sort %s -o merged.bam`", len(several), " ".join(several))
            raise SystemExit(1)
        # (SAM text under SVX_DEVICE_SORT=write / =1 takes the road of an unsorted BAM; every other setting reads it as a BAM and refuses it)
        head = None if several or piped or switch in ("write", "1") and _is_sam_text(options.bam_path) else read_bam_header(options.bam_path)
        if head is not None and head.sort_order == "coordinate":
            fasta = Fasta(options.genome)
            index = find_index(options.bam_path)
            # (SVX_BUILD_INDEX=1: a .bai; =csi: a .csi, the format for positions from 2^29 on -- "bai" / "csi", or False)
            build_index = index is None and {"1": "bai", "csi": "csi"}.get(os.environ.get("SVX_BUILD_INDEX"), False)
            if build_index and ws > 1:
                # (every rank would build the same file; one build in front of the launch serves them all)
                logging.error("SVX_BUILD_INDEX=%s builds the index in a single-rank run only: build it first with "
                              "`python -m svision_amd.index %s%s` and start the %d ranks again", os.environ["SVX_BUILD_INDEX"],
                              "--csi " if build_index == "csi" else "", options.bam_path, ws)
                raise SystemExit(1)
            return RunInput(None, fasta, head.references, head.lengths, index, build_index)
        if os.environ.get("SVX_DEVICE_SORT") == "write":
            if ws > 1:
                # (every rank would write the same file; one sort in front of the launch serves them all)
                logging.error("SVX_DEVICE_SORT=write sorts an unsorted BAM in a single-rank run only: write the sorted file first with "
                              "`python -m svision_amd.sort %s -o sorted.bam` and start the %d ranks on it", " ".join(several or [options.bam_path]), ws)
                raise SystemExit(1)
            options.bam_path = _write_sorted(options)
            tick("unsorted BAM: sorted file written on the device")
            return _open_input(options, None, ws, tick)             # the ordinary file-driven run on the sorted, indexed file
        if os.environ.get("SVX_DEVICE_SORT") != "1":
            logging.error("This is not a coordinate sorted BAM file")
            logging.error("(SVX_DEVICE_SORT=1 sorts its records on the device: one rank, the whole file resident)")
            raise SystemExit(1)
        if ws > 1:
            # (every rank would read and sort the whole file; the ranks share chromosomes, not records in file order)
            logging.error("SVX_DEVICE_SORT=1 sorts an unsorted BAM in a single-rank run only: sort and index %s first "
                          "(`samtools sort`, then `python -m svision_amd.index`) and start the %d ranks again", " ".join(several or [options.bam_path]), ws)
            raise SystemExit(1)
        sample = _load_unsorted(options, several)
        tick("unsorted BAM: records sorted on the device")
        if several or piped:                                        # a stable name for the run: ``stdin``, the first input of a list
            options.bam_path = "stdin" if (several or [options.bam_path])[0] == "-" else (several or [options.bam_path])[0]
    _sample.register(options.bam_path, sample)
    return RunInput(sample, sample.fasta, sample.table.references, sample.table.lengths, None, False)


def _plan(options, inp, rank, ws):
    """Plan step.  Needs the RunInput; sets ``options.min_support`` to 1 under ``--contig``.  -> (tasks {chrom: [[start, end], ...]} of
    the whole run, this rank's chromosomes in task order); SystemExit(1) when no reference of the BAM is in the FASTA."""
    if options.contig:
        options.min_support = 1
    tasks = build_tasks(options, inp.references, inp.lengths, inp.fasta.references)
    if len(tasks) == 0:
        logging.error("No mapped reads in the BAM, please check your reference input!")
        raise SystemExit(1)
    return tasks, _rank_shard(list(tasks), inp.references, inp.lengths, rank, ws)


class _DeviceRun:
    """What the streamed device path holds open: the feed the windows' records come from and, for ``-t N`` on a file, the helpers
    forked for it.  ``close`` releases what has been set up so far (both closes may be called again: PooledHotPath closes the pool too)."""
    feed = pool = None

    def close(self):
        try:
            if self.feed is not None:
                self.feed.close()
        finally:
            if self.pool is not None:
                self.pool.close()


def _set_up_device(dev, options, inp, tasks, mine, dirs, rank, ws, tick):
    """Device set-up step.  Needs the RunInput and the plan; fills ``dev.pool`` and ``dev.feed`` as they come up, in this order: helpers
    forked (before the first HIP call), this rank's GPU selected, the process group, the index built where asked, the feed.  A
    Sample sorted on the device has touched it already: no fork here, PooledHotPath makes its own pool."""
    if options.thread_num > 1 and inp.sample is None:
        # -t N: fork the host helpers before the first HIP call (pipeline.HelperPool); they map every chromosome
        # from shared memory when the feed announces it
        from .pipeline import HelperPool
        dev.pool = HelperPool(options.thread_num, options, fasta=inp.fasta, want_tsv=True)
    from .build_host import compiled_state
    _compiled, _interp = compiled_state()
    if _interp:
        logging.warning("host modules running interpreted (2-4x slower collection and vote): %s -- build them with `python -m svision_amd.build_host`", ", ".join(_interp))
    tick("header, FASTA index, fork helpers")
    # one process per GPU: every device tensor of this rank (scan buffers, weights, graphs) lives on its own GPU.
    # The process group comes up now (after the fork, before the first long phase), not when the first rank is done:
    # a late rendezvous would time out whenever the shards finish far apart.
    import torch
    if torch.cuda.is_available():
        torch.cuda.set_device(sdist.local_device_index())
    sdist.init_from_env()
    from .ingest import ChromosomeFeed, StaticFeed, decode_threads
    if inp.sample is not None:
        dev.feed = StaticFeed(inp.sample)
        return
    index, device = inp.index, torch.device("cuda", torch.cuda.current_device())
    threads = decode_threads(int(os.environ.get("LOCAL_WORLD_SIZE", ws)), options.thread_num)      # inflate threads of this rank
    if inp.build_index:
        # SVX_BUILD_INDEX=1 (=csi: a .csi) and no index next to the BAM: built on the device (svision_amd/index.py) into the output directory --
        # the BAM's own may be read-only --, and the device engine serves the run
        from .index import build_index
        index = build_index(options.bam_path, os.path.join(dirs.out_path, os.path.basename(options.bam_path) + "." + inp.build_index), device=device,
                            **(dict(fmt="csi") if inp.build_index == "csi" else {}))
        logging.info("no index next to %s: built %s on the device", options.bam_path, index)
        tick("index built on the device")
    dev.feed = ChromosomeFeed(options.bam_path, inp.fasta, options, [c for c in mine if c in inp.references], inp.references, inp.lengths,
                              device=device, index=index, threads=threads, tasks={c: tasks[c] for c in mine if c in tasks})
    logging.info("rank %d/%d: %s streamed from %s with %d decode threads", rank, ws, ",".join(mine) or "-", options.bam_path, threads)


def _begin_work(dirs):
    """segments/ and predict_results/ exist -> the time the compute step began."""
    os.makedirs(dirs.segments, exist_ok=True)
    os.makedirs(dirs.predict_results, exist_ok=True)
    return datetime.datetime.now()


def _compute_streamed(options, inp, tasks, mine, dirs, rank, ws, tick):
    """Compute step of the device path, with its set-up: Step 1 and Step 2 streamed window by window (collection of window k+1 on the
    host while the device classifies window k), one vote stream per chromosome in window order = the order of all.bed.  Leaves this
    rank's score.txt and .vcf per chromosome; the feed and the helpers are closed however it ends.  -> when the compute began."""
    dev = _DeviceRun()
    try:
        _set_up_device(dev, options, inp, tasks, mine, dirs, rank, ws, tick)
        t0 = _begin_work(dirs)
        if options.thread_num > 1:
            _run_pooled(options, dev.feed, tasks, mine, dirs.segments, dirs.predict_results, dev.pool)
        else:
            _run_streaming(options, dev.feed, tasks, mine, dirs.segments, dirs.predict_results)
    finally:
        dev.close()
    if tick.on and hasattr(dev.feed, "stats"):
        print("ingest: %s" % {k: (round(v, 3) if isinstance(v, float) else v) for k, v in dev.feed.stats.items()}, flush=True)
    logging.info("[Coding + prediction finished]: streamed, Cost time: %s", (datetime.datetime.now() - t0).seconds)
    return t0


def _compute_from_files(options, sample, classifier, tasks, mine, dirs):
    """Compute step with an injected classifier, as upstream runs it: Step 1 writes every window's part bed and joins them to all.bed,
    Step 2 predicts from all.bed.  Needs the registered Sample.  Leaves what the device path leaves.  -> when the compute began."""
    from .collection import run_collection
    from .network.predict import Predict
    t0 = _begin_work(dirs)
    logging.info("\n****************** Step1 Image coding and segmentation ******************")
    for chrom in mine:
        with open(dirs.all_bed(chrom), "w") as out:              # `cat parts > all.bed`
            for part, (start, end) in enumerate(tasks[chrom]):
                err = run_collection.run_detect(options, options.bam_path, chrom, part, start, end)
                if err is not None:
                    logging.error("%s:%s-%s %s", chrom, start, end, err)      # upstream drops this string silently
                if os.path.exists(dirs.part_bed(chrom, part)):
                    with open(dirs.part_bed(chrom, part)) as f:
                        shutil.copyfileobj(f, out)
    t1 = datetime.datetime.now()
    logging.info("[Coding finished]: Collect segment signatures, Cost time: %s", (t1 - t0).seconds)

    logging.info("\n****************** Step2 CNN prediction ******************")
    for chrom in mine:
        Predict(chrom, dirs.all_bed(chrom)).run(dirs.predict_prefix(chrom), options, classifier=classifier, sample=sample)
    logging.info("[Prediction finished]: Predicting types, Cost time: %s", (datetime.datetime.now() - t1).seconds)
    return t0


def _exchange(options, dirs, mine, rank, ws):
    """The single cross-shard exchange.  Needs this rank's score.txt and .vcf files (and graphs/ under ``--graph``).  -> (max score,
    min score, whether a process group carried it); on rank 0 predict_results/ and graphs/ then hold every rank's texts.  Prints
    and leaves with SystemExit(0) when no rank has a score."""
    from .network.output import cal_scores_max_min
    sdist.init_from_env()
    local_scores = cal_scores_max_min(dirs.predict_results) if ws == 1 else _scores_of(dirs, mine)
    max_score, min_score = sdist.exchange_score_range(local_scores)
    if max_score is None:
        print("Empty output in the score file!!! Program exit")
        raise SystemExit(0)
    grouped = sdist.world_initialized()      # ws > 1, or one rank with SVX_FORCE_DIST=1 (the RCCL path on a one-GPU box)
    if not grouped:
        return max_score, min_score, grouped
    bodies = {}
    for chrom in mine:
        with open(dirs.predict_vcf(chrom)) as f:
            bodies[chrom] = f.read()
    bodies = sdist.gather_texts(bodies, dst=0)
    if rank == 0:
        for chrom, text in bodies.items():
            with open(dirs.predict_vcf(chrom), "w") as f:
                f.write(text)
    if options.graph:
        # the per-read graphs of a reported cluster are written by the rank that collected it (graphs/{chrom}-{start}-{end}/
        # {read}.gfa); step 3 runs on rank 0, and the out_path need not be a filesystem the ranks share: the
        # graph texts travel with the VCF bodies
        mine_set, texts = set(mine), {}
        for name in sorted(os.listdir(dirs.graphs)):
            d = os.path.join(dirs.graphs, name)
            if os.path.isdir(d) and name.rsplit("-", 2)[0] in mine_set:
                for fn in sorted(os.listdir(d)):
                    with open(os.path.join(d, fn)) as f:
                        texts[name + "/" + fn] = f.read()
        texts = sdist.gather_texts(texts, dst=0)
        if rank == 0:
            for rel, text in texts.items():
                path = os.path.join(dirs.graphs, rel)
                if not os.path.exists(path):
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                    with open(path, "w") as f:
                        f.write(text)
    return max_score, min_score, grouped


def _merge(options, dirs, fasta, chroms, max_score, min_score, grouped, rank, t0, tick):
    """Merge step.  Rank 0 merges the chromosomes' VCFs (and under ``--graph`` runs Step 3, which replaces the plain VCF by the
    graph VCF); the ranks of a group meet at a barrier; rank 0 removes segments/ and predict_results/ unless ``--debug``.
    -> the path of the merged VCF on rank 0, None elsewhere."""
    merged_path = None
    if rank == 0:
        from .network.output import merge_split_vcfs
        merged_path = dirs.merged_vcf()
        options.source_version = REFERENCE_VERSION
        merge_split_vcfs(dirs.predict_results, merged_path, max_score, min_score, chroms, options, fasta=fasta)
        if options.graph:                    # SVision:341-359: graph VCF + summaries; the plain VCF and the per-site folders go
            from .collection.graph import annotate_vcf_with_graphs
            logging.info("\n****************** Step3 Computing graphs ******************")
            annotate_vcf_with_graphs(dirs.graphs, merged_path, options)
            for name in os.listdir(dirs.graphs):
                if os.path.isdir(os.path.join(dirs.graphs, name)):
                    shutil.rmtree(os.path.join(dirs.graphs, name))
            os.remove(merged_path)
            merged_path = dirs.merged_vcf(graph=True)
            logging.info("[Graph creation finished] Generate graphs")
        logging.info("[All steps finished] Total Cost time: %ss", (datetime.datetime.now() - t0).seconds)
    tick("exchange + merge")
    if grouped:
        import torch.distributed as tdist
        if tick.on:
            print("exchange backend %s, world %d" % (tdist.get_backend(), tdist.get_world_size()), flush=True)
        logging.info("cross-rank exchange over %s, world size %d", tdist.get_backend(), tdist.get_world_size())
        tdist.barrier()
    if not options.debug and rank == 0:
        shutil.rmtree(dirs.segments, ignore_errors=True)
        shutil.rmtree(dirs.predict_results, ignore_errors=True)
    return merged_path


def run(options, sample=None, classifier=None):
    """Whole pipeline; returns the merged VCF path (rank 0) or None.  ``sample``: a resident Sample in place of the file's records;
    ``classifier``: the file-based Step 1 + Step 2 with this classifier in place of the streamed device path.  The run's log
    handler, the feed and the helpers are released whichever way it is left."""
    rank, ws = sdist.env_rank()              # the process group comes up after the host helpers are forked (_set_up_device)
    dirs = RunDirs(options)
    os.makedirs(dirs.out_path, exist_ok=True)
    if options.graph:                        # SVision:253-256; before the helpers are forked: they write the per-read graphs
        os.makedirs(dirs.graphs, exist_ok=True)
    with _run_log(dirs.out_path, rank, ws):
        logging.info("******************** Start SVision, version %s (svision_amd %s) ********************", REFERENCE_VERSION, __version__)
        logging.info("CMD: %s", " ".join(sys.argv))
        logging.info("WORKDIR DIR: %s", os.path.abspath(dirs.out_path))
        logging.info("CNN MODEL: %s", os.path.abspath(options.model_path))
        logging.info("INPUT BAM: %s", options.bam_path)
        tick = _Ticker()
        inp = _open_input(options, sample, ws, tick)
        tasks, mine = _plan(options, inp, rank, ws)
        if classifier is None:
            t0 = _compute_streamed(options, inp, tasks, mine, dirs, rank, ws, tick)
        else:
            t0 = _compute_from_files(options, inp.sample, classifier, tasks, mine, dirs)
        tick("collection + encode + CNN + vote")
        max_score, min_score, grouped = _exchange(options, dirs, mine, rank, ws)
        return _merge(options, dirs, inp.fasta, list(tasks), max_score, min_score, grouped, rank, t0, tick)


def _run_streaming(options, feed, tasks, chroms, seg_dir, pred_dir):
    """Steps 1 + 2 without the TSV round trip: same functions, same order of lines, same vote semantics as
    Predict.run over ``{chrom}.segments.all.bed`` (predict.py:206-300); the segment files are still written."""
    import traceback
    from .network.predict import Predict, SiteVoter, load_network
    from .pipeline import HotPath
    dirs, clock = RunDirs(options, seg_dir, pred_dir), _Ticker()
    net = load_network(options.model_path)
    hot = HotPath(None, options, net, n_streams=3, lazy_graphs=True)      # a command line captures the launch shapes it meets (pipeline.DeviceStage)
    set_up = clock.lap()
    for chrom in chroms:
        with _chromosome_files(dirs, chrom) as (score_out, vcf_out, write_part):
            voter = SiteVoter(Predict(chrom, None), vcf_out, score_out, options, None)
            logging.info("Predicting " + chrom)

            def feed_votes(res):
                classes, probs = hot.fetch_predictions(res)
                voter.next_sample = res.sample                    # a site is written on the records of the window that opened it
                voter.feed_batch([ln.label() for ln in res.lines], classes, probs)

            prev = None
            for part, (start, end) in enumerate(tasks[chrom]):
                # waits for the window's records (decoded ahead; the device engine hands a chromosome over in slices of windows)
                _key, hot.sample = feed.get(chrom, block=True, start=start)
                try:
                    cur = hot.collect(chrom, start, end, rescan=False)
                except Exception:                                 # run_collection.py:44-47: the window yields nothing
                    _t, value, trace = sys.exc_info()
                    logging.error("%s:%s-%s [ERROR]: %s. Locate At: %s", chrom, start, end, value, traceback.extract_tb(trace))
                    cur = hot.empty(chrom, start, end)
                cur.sample = hot.sample
                write_part(part, "".join(ln.text() for ln in cur.lines))
                if prev is not None:
                    feed_votes(prev)
                prev = hot.launch(cur)
            if prev is not None:
                feed_votes(prev)
            voter.finish()
        feed.release(chrom)
    if clock.on:
        print("network + graphs %.3f, windows %.3f" % (set_up, clock.lap()), flush=True)


def _run_pooled(options, feed, tasks, chroms, seg_dir, pred_dir, pool=None):
    """``-t N`` (the reference's process-pool size, SVision:261,311): N forked helper processes run the collection and
    the vote of whole windows while this process feeds the device (pipeline.PooledHotPath); windows complete in any
    order; a chromosome is stitched and written (in task order inside it) as soon as its last window is done, so the
    files are those of the one-process path and only the chromosomes in flight are resident."""
    from .network.predict import load_network
    from .pipeline import PooledHotPath, stitch_windows
    net = load_network(options.model_path)
    windows = [(chrom, start, end) for chrom in chroms for start, end in tasks[chrom]]
    first = {}
    for wid, (chrom, _s, _e) in enumerate(windows):
        first.setdefault(chrom, wid)
    left = {chrom: len(tasks[chrom]) for chrom in chroms}
    dirs, clock = RunDirs(options, seg_dir, pred_dir), _Ticker()
    static = getattr(feed, "sample", None)
    hot = PooledHotPath(static, options, net, n_workers=options.thread_num, n_streams=3, max_inflight=6, want_tsv=True, pool=pool, feed=feed, lazy_graphs=True)
    pool_up = clock.lap()
    done = {}

    def write_chromosome(chrom):
        wids = range(first[chrom], first[chrom] + len(tasks[chrom]))
        texts = stitch_windows([done[w] for w in wids], options,               # per-chromosome vote: edge sites written once
                               lambda c, start: feed.get(c, block=True, start=start)[1])
        vcf_text, score_text = texts.get(chrom, ("", ""))
        logging.info("Predicting " + chrom)
        with _chromosome_files(dirs, chrom) as (score_out, vcf_out, write_part):
            for part, w in enumerate(wids):
                write_part(part, done.pop(w).tsv)
            vcf_out.write(vcf_text)
            score_out.write(score_text)
        hot.release(chrom)

    try:
        for res in hot.run_windows(windows, rescan=False):
            done[res.wid] = res
            left[res.chrom] -= 1
            if left[res.chrom] == 0:
                write_chromosome(res.chrom)
    finally:
        in_windows = clock.lap()
        hot.close()
    for chrom in chroms:                                          # chromosomes without a window (cannot happen) or never reached
        if left[chrom] and not os.path.exists(dirs.predict_vcf(chrom)):
            raise RuntimeError("chromosome %s was not completed" % chrom)
    if clock.on:
        print("pool up %.3f, windows %.3f, close %.3f, owner %s" % (pool_up, in_windows, clock.lap(),
              {k: round(v, 3) for k, v in getattr(hot, "owner_profile", {}).items()}), flush=True)


@contextlib.contextmanager
def _chromosome_files(dirs, chrom):
    """The files the compute step leaves for one chromosome, open for writing -> (score.txt, .vcf, write_part); ``write_part(part, text)``
    writes a window's segment signatures to its part bed and to all.bed, so the windows are to be given in task order."""
    with open(dirs.score_txt(chrom), "w") as score_out, open(dirs.predict_vcf(chrom), "w") as vcf_out, open(dirs.all_bed(chrom), "w") as all_bed:
        def write_part(part, text):
            with open(dirs.part_bed(chrom, part), "w") as f:
                f.write(text)
            all_bed.write(text)
        yield score_out, vcf_out, write_part


def _scores_of(dirs, chroms):
    """Scores of this rank's chromosomes only (a shared out_path may hold other ranks' files)."""
    scores = []
    for chrom in chroms:
        path = dirs.score_txt(chrom)
        if os.path.exists(path):
            with open(path) as f:
                scores += [float(l.strip()) for l in f if l.strip() != "0"]
    return scores


def main(arguments=None):
    options = parse_arguments(arguments)
    if options.hash and os.environ.get("SVX_HASH_LONG", "1") != "0":
        # pieces of up to 65,536 bases (--max_hash_len raised) re-align on the device too (svx_hash_seeds_long); a process
        # global like DEVICE and REMOTE, set here, before run() forks the helpers (SVX_HASH_LONG=0: the host aligner, as before)
        from . import kernels
        from .segmentplot import run_hash_lineplot
        run_hash_lineplot.MAX_PIECE = kernels.HASH_LONG_MAX_X
    run(options)


if __name__ == "__main__":
    main()
