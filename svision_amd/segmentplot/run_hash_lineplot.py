"""``hashplot_unmapped``: place an unmapped / inserted read piece on its local reference window.

Mirror of the reference's src/segmentplot/run_hash_lineplot.py (``hashplot_unmapped`` :52-85,
``select_longest`` :8-33).  ``cord_to_segments`` lives in :mod:`.classes`.
"""
import os

from .classes import Segment, cord_to_segments  # noqa: F401  (re-exported like upstream)
from .hash_aligner import HashAligner


def select_longest(segments):
    """Longest hit(s) per strand, forward ones first (:8-33)."""
    best = {True: [], False: []}
    for seg in segments:
        bucket = best[seg.forward() == True]      # noqa: E712  (None counts as reverse, as upstream)
        span = abs(seg.xEnd() - seg.xStart())
        if not bucket or span > abs(bucket[0].xEnd() - bucket[0].xStart()):
            bucket[:] = [seg]
        elif span == abs(bucket[0].xEnd() - bucket[0].xStart()):
            bucket.append(seg)
    return best[True] + best[False]


DEVICE = None        # torch.device of the process that owns a GPU (set by Sample.from_table); None in the forked host helpers
MAX_PIECE = None     # longest piece the device takes: None = the short kernel's kernels.HASH_MAX_X; a --hash run of the command line sets
                     # kernels.HASH_LONG_MAX_X before the helpers fork (svx_hash_seeds_long), SVX_HASH_LONG=0 leaves it None
REMOTE = None        # in a host helper: callable (bases, desc, k, window) -> (counts, row_off, rows) or None, the owner's device by pipe (pipeline._Helper.remote_hash)


def batch_enabled():
    """SVX_HASH_BATCH=0: the collection re-aligns piece by piece where the pieces arise (a launch per job in the process that
    owns the device, the host aligner in the helpers) instead of a window's pieces together.  Read at call time."""
    return os.environ.get("SVX_HASH_BATCH", "1") != "0"


def hashplot_unmapped(ref, seq, k, min_accept):
    """-> (None, segments): self-align the window to learn its repeats, then place ``seq`` (:52-85).
    In the GPU-owning process the two seed-and-extend passes run on the device (``svx_hash_seeds``); the hit lists
    are replayed through the same order-dependent host steps.  Sequences outside the alphabet ACGTN (upstream's
    k-mers are raw strings), pieces longer than the kernels take (``MAX_PIECE``), k > 13 and overflowing hit lists take the host
    passes below, which are also what the helper processes (no GPU) run."""
    if DEVICE is not None:
        got = hashplot_unmapped_batch([(ref, seq)], k, min_accept, DEVICE)[0]
        if got is not None:
            return None, got
    return None, _hashplot_host(ref, seq, k, min_accept)


def _hashplot_host(ref, seq, k, min_accept):
    repeat_thresh = 2
    self_pass = HashAligner(k, min_accept, 0, repeat_thresh)
    self_pass.run(ref, ref)
    placer = HashAligner(k, min_accept, 0, repeat_thresh)
    placer.run(seq, ref, self_pass.getSelfDiffSegs(), self_pass.getHashValues(), self_pass.getAvoidKmer())
    merged = placer.getMergeSegments()
    if len(merged) >= 2:
        merged = select_longest(merged)
    return merged


def hashplot_unmapped_many(pairs, k, min_accept):
    """[(ref, seq), ...] -> [segments]: what :func:`hashplot_unmapped` gives for every pair, all pairs the device takes in one
    batch (on ``DEVICE``, or on the owner's through ``REMOTE``), the others through the host passes in this process."""
    got = hashplot_unmapped_batch(pairs, k, min_accept, DEVICE)
    return [_hashplot_host(ref, seq, k, min_accept) if segs is None else segs for segs, (ref, seq) in zip(got, pairs)]


def _replay(hits_a, hits_b, x_len, y_len, k, min_accept):
    """The device's two raw hit lists of one job -> its segments, through the order-dependent host steps."""
    self_pass = HashAligner(k, min_accept, 0, 2)
    self_pass.compareDiffSegs = None
    for i, pos, length, fwd in hits_a.tolist():          # the self pass: its off-diagonal hits are the window's repeats
        self_pass._keep(Segment(pos, i, length, True, 0) if fwd else Segment((y_len - 1) - pos, i, length, False, 0))
    placer = HashAligner(k, min_accept, 0, 2)
    placer.compareDiffSegs = self_pass.getSelfDiffSegs()
    for i, pos, length, fwd in hits_b.tolist():
        placer._keep(Segment(pos, i, length, True, 0) if fwd else Segment((x_len - 1) - pos, i, length, False, 0))
    merged = placer.getMergeSegments()
    if len(merged) >= 2:
        merged = select_longest(merged)
    return merged


def hashplot_unmapped_batch(pairs, k, min_accept, device):
    """[(ref, seq), ...] -> [segments or None]: every pair's seed-and-extend passes in ONE call of the device executor
    (``kernels.hash_seeds``; with ``device`` None in a helper process, the owner's executor through ``REMOTE``).
    None = the pair cannot go through the device kernel (see :func:`hashplot_unmapped`), or there is no device to ask."""
    from .. import kernels
    out = [None] * len(pairs)
    jobs, where = [], []
    if not (2 <= k <= 13) or (device is None and REMOTE is None):
        return out
    longest = kernels.HASH_MAX_X if MAX_PIECE is None else MAX_PIECE
    more = {} if MAX_PIECE is None else {"max_piece": MAX_PIECE}
    for n, (ref, seq) in enumerate(pairs):
        if len(seq) > longest:
            continue
        x, y = kernels.pack_bases(seq), kernels.pack_bases(ref)
        if x is None or y is None:
            continue
        jobs.append((x, y))
        where.append(n)
    if device is not None:
        results = kernels.hash_seeds(jobs, k, min_accept, device, **more)
    elif jobs:
        bases, desc = kernels.hash_job_arrays(jobs)
        lists = REMOTE(bases, desc, k, min_accept)
        if lists is None:                                      # the owner could not run them: every pair takes the host passes
            return out
        results = kernels.hash_split_rows(desc, *lists)
    else:
        results = []
    for n, res, (x, y) in zip(where, results, jobs):
        if res is not None:
            out[n] = _replay(res[0], res[1], len(x), len(y), k, min_accept)
    return out
