"""Crafted BGZF blocks with long literal runs and long matches for bgzf_lz_table_kernel (csrc/svx_lz_table.hip), from explicit
tokens (tests/deflate_writer.py): runs around 16, 32 and 64 entries (the thresholds tools/hostwave/lz_table_main.cpp --count
counts a wave-cooperative build at), around the wave's 64 lanes and up to the longest a sequence holds, and where in a wave and a
batch of the build they fall.  Shared by test_gpu_lz_table_runs.py (the kernel) and test_lz_table_runs_cpu.py (the same phase
code on the host under the sanitizers, and the turn counts of --count).

How tokens become sequences (bgzf_tokens_kernel<true>): a match closes a sequence [literals in front of it | match]; a run of
literals is also closed at 255 bytes, at the end of a DEFLATE block and where a lane segment of 512 compressed bits ends.  So
  * a stored DEFLATE block of n <= 255 bytes is exactly one literal-only sequence of n, one of 600 bytes is 255 + 255 + 90;
  * n <= 255 literals of a two-symbol alphabet with code lengths 1 and 2, first in a dynamic block, take < 512 bits: followed
    by a match they are one sequence [n | match];
  * every match token is a sequence of its own (with the literals in front of it)."""
import zlib

import numpy as np

from tests import deflate_writer as dw

BAD_DIST = 8                                                   # svx_lz_table_core.hpp: LZ_BAD_DIST
LONG = 32                                                      # a "long" part in the cases below


def run_lengths(cap):
    return [n for n in (15, 16, 17, 31, 32, 33, 63, 64, 65, 254, 255, 256, 258, 600) if n <= cap]


def _rand(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def _two_symbol_run(n):
    """n literals, 'a' but every seventh 'b' (7 does not divide 64: a lane that took another lane's literal shows)."""
    return [98 if k % 7 == 3 else 97 for k in range(n)]


class Case:
    def __init__(self, name, d, status=0, isize=None, data=None):
        self.name, self.status = name, status
        self.data = bytes(d.data) if data is None else data
        self.block = dw.bgzf(d.getvalue(), self.data, isize=isize)
        if status == 0:
            assert zlib.decompress(d.getvalue(), -15) == self.data, name          # zlib is the reference


def build():
    """-> [Case], the good ones with .data = zlib's bytes, the malformed one with .status = the code its block must get."""
    rng = np.random.default_rng(31)
    r = LONG
    cases = []
    # literal-only sequences of every length (a stored block each; 256 = 255 + 1, 600 = 255 + 255 + 90)
    d = dw.Deflate()
    for n in run_lengths(600):
        d.stored(_rand(rng, n))
    d.fixed([], final=True)
    cases.append(Case("literal_runs_stored", d))
    # [n literals | match of m] in one sequence: either part short or long
    d = dw.Deflate()
    pairs = [(n, m) for n in run_lengths(255) for m in (3, r)] + [(r - 1, r - 1), (255, 258), (1, 258)]
    for k, (n, m) in enumerate(pairs):
        d.dynamic(_two_symbol_run(n) + [(m, 1 + k % n)], final=k == len(pairs) - 1)
    cases.append(Case("literal_run_then_match", d))
    # matches of every length: fully overlapping, distance = length, the furthest distance DEFLATE has
    d = dw.Deflate()
    d.fixed([120] + [(m, 1) for m in run_lengths(258)], final=True)
    cases.append(Case("matches_distance_1", d))
    d = dw.Deflate()
    d.stored(_rand(rng, 300))
    d.fixed([(m, m) for m in run_lengths(258)], final=True)
    cases.append(Case("matches_distance_is_length", d))
    d = dw.Deflate()
    d.stored(_rand(rng, 32768))                                   # (a stored block in front of a compressed one)
    d.fixed([(m, 32768) for m in run_lengths(258)], final=True)
    cases.append(Case("matches_distance_32768", d))
    # a wave whose 64 sequences are all long (two of them: sequences 0 .. 127)
    d = dw.Deflate()
    d.stored(_rand(rng, 100))
    d.fixed([(r + k % 5, 1 + 7 * k % 100) for k in range(128)], final=True)
    cases.append(Case("all_64_lanes_long", d))
    # exactly one long sequence in a wave: lane 0 of the first wave, lane 63 of the second
    cases.append(Case("long_in_lane_0_and_lane_63", lane_0_and_63()))
    # the last sequence of a batch (index 1,023) and the first of the next (1,024) long
    d = dw.Deflate()
    d.fixed([65, 66, (3, 2)] + [(3, 1 + k % 5) for k in range(1022)] + [(258, 258), (255, 1), (3, 3)], final=True)
    cases.append(Case("long_across_the_batch_border", d))
    # exactly 0xFF00 bytes ending in a long match / in a 255-literal sequence (0xFF00 = 256 x 255)
    d = dw.Deflate()
    d.stored(_rand(rng, 0xFF00 - 258))
    d.fixed([(258, 300)], final=True)
    cases.append(Case("isize_0xff00_ends_in_a_long_match", d))
    d = dw.Deflate()
    d.stored(_rand(rng, 0xFF00), final=True)
    cases.append(Case("isize_0xff00_ends_in_255_literals", d))
    # malformed: a long match that starts one byte in front of the block
    d = dw.Deflate()
    d.fixed([65] * 10 + [(100, 11)], final=True)
    cases.append(Case("long_match_in_front_of_the_block", d, status=BAD_DIST, isize=110, data=b"A" * 110))
    return cases


def stored_600():
    """255 + 255 + 90 literals, nothing else: one wave, three parts that are long at every threshold."""
    d = dw.Deflate()
    d.stored(_rand(np.random.default_rng(5), 600), final=True)
    return d


def lane_0_and_63():
    """Sequences 0: [1 | 100], 1 .. 63: [0 | 3], 64 .. 126: [0 | 3], 127: [0 | 200]."""
    d = dw.Deflate()
    d.fixed([120, (100, 1)] + [(3, 1)] * 63 + [(3, 2)] * 63 + [(200, 5)], final=True)
    return d


def filler(n, seed):
    d = dw.Deflate()
    d.stored(_rand(np.random.default_rng(seed), n), final=True)
    return dw.bgzf(d.getvalue(), bytes(d.data)), bytes(d.data)


def at_phase(cases, phase):
    """-> [(block, bytes it must give or None, status)]: in front of every case a filler that puts the case's output at an address
    ``phase`` mod 16 (the launch's output starts at a multiple of 16)."""
    out, at = [], 0
    for k, c in enumerate(cases):
        n = (phase - at) % 16 or 16
        fb, fd = filler(n, 100 + k)
        out.append((fb, fd, 0))
        at += n
        assert at % 16 == phase
        out.append((c.block, c.data if c.status == 0 else None, c.status))
        at += len(c.data)
    fb, fd = filler(33, 99)                                       # (the malformed block has a neighbour behind it too)
    out.append((fb, fd, 0))
    return out
