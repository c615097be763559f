"""The catalogue of --hash re-aligner cases with pieces of more than 2,048 bases (svx_hash_seeds_long: x's k-mer entries in
tiles of 4,096), in the style of tests/hashcases.py and from its helpers: shared by the script that records the reference's
answers (tests/golden/make_hash_long_fixture.py), the CPU test (tests/test_hash_long_cpu.py) and the GPU tests
(tests/test_gpu_hash_long.py).

A case is a ``hashcases.Case``; the name starts with ``l/``, except the one-tile case, which is ``hashcases.TOO_LONG`` itself.
Every sequence is a function of the case's name alone.  The entries of a piece of ``n`` bases at k: e = 0 .. 2 (n - k - 1) - 1,
forward positions first, then those of the reverse complement; tile t holds e = 4096 t .. 4096 t + 4095."""
import gzip
import json
import os

from tests import hashcases as hc
from tests.hashcases import Case, _COMP, _rng, mutate_every, other, rc, rs

TILE = 4096
LONG_MAX_X = 65536                               # the tiled kernel's longest piece
EDGE_PARAMS = hc.FULL_PARAMS                     # (2, 2), (10, 50), (13, 50)
STRAND = "l/strand3000/k10w50"
ONE_Y = "l/one-y-three-tiles/k10w50"
CHUNK_EDGE = "l/y255-257-tile1/k10w50"
OVERFLOW = "l/overflow/k2w2"
ALPHABET = "l/wide4000/k10w30"
SIX_TILES = "l/piece12000/k10w50"
LONGEST = "l/piece65536/k10w50"
TOO_LONG = "l/piece65537/k10w50"


def entries(case):
    return 2 * max(0, len(case.seq) - (case.k + 1))


def tile_of(case, pos, forward):
    """The tile that holds the entry of x position ``pos`` (forward) / of position ``pos`` in x's reverse complement."""
    nx = len(case.seq) - (case.k + 1)
    return (pos if forward else nx + pos) // TILE


# ---- the tile edge: exactly 4096 entries, and two entries more ------------------------------------------------------------------
def _edge_k2(name, total):
    """k = 2, window = 2 on "ACAAAAA" ("AC" occurs once on either strand; "T" filler only makes avoided k-mers): "AC" planted
    forward at the first, a middle and the last two forward entries, "GT" so that its reverse-strand "AC" falls on the last
    entry of the first tile (x[4:6]) and on the very last entry (x[2:4])."""
    nx = total - 3
    x = ["T"] * total
    for p in (0, 1000, nx - 3, nx - 1):
        x[p:p + 2] = "AC"
    x[2:4] = "GT"
    x[4:6] = "GT"
    x[1500:1502] = "GT"
    return Case(name, "ACAAAAA", "".join(x), 2, 2)


def edge_cases():
    out = []
    for k, window in EDGE_PARAMS:
        for extra in (0, 1):
            total = hc.MAX_X + k + 1 + extra                              # 2 (total - k - 1) = 4096 entries, or 4098
            name = "l/edge%d/k%dw%d" % (2 * (total - k - 1), k, window)
            if k == 2:
                out.append(_edge_k2(name, total))
                continue
            rng = _rng(name)
            ref = rs(rng, 3000)
            out.append(Case(name, ref, hc._three_copies(rng, ref, total), k, window))
    return out


# ---- the strand boundary inside the first tile -------------------------------------------------------------------------------------
def strand_cases():
    rng = _rng(STRAND)
    ref = rs(rng, 4000)
    return [Case(STRAND, ref, hc._three_copies(rng, ref, 3000), 10, 50)]


# ---- one y position, hits in three tiles, both strands -----------------------------------------------------------------------------
ONE_Y_FWD = (100, 4500)                          # x positions of u: tiles 0 and 1
ONE_Y_REV = (3000, 1000)                         # x positions of rc(u): reverse-strand positions 1930 and 3930, tiles 1 and 2


def one_y_cases():
    rng = _rng(ONE_Y)
    u = rs(rng, 70)
    ref = rs(rng, 300) + u + rs(rng, 300)
    x = list(rs(rng, 5000))
    for p in ONE_Y_FWD:
        x[p - 1] = other(rng, ref[299])                                   # the seed rule looks at the base in front
        x[p:p + 70] = u
    for p in ONE_Y_REV:
        x[p:p + 70] = rc(u)
        x[p + 70] = _COMP[other(rng, ref[299])]
    return [Case(ONE_Y, ref, "".join(x), 10, 50)]


# ---- y chunks of 256 against tiles ---------------------------------------------------------------------------------------------------
def chunk_cases():
    rng = _rng(CHUNK_EDGE)
    ref = rs(rng, 1500)
    tail = ref[255:315] + other(rng, ref[255]) + ref[256:316] + other(rng, ref[256]) + ref[257:317] + rs(rng, 40)
    lead = rs(rng, 4199) + other(rng, ref[254])
    return [Case(CHUNK_EDGE, ref, lead + tail, 10, 50)]


# ---- overflow, alphabet, larger shapes -------------------------------------------------------------------------------------------------
def overflow_cases():
    return [Case(OVERFLOW, "ACAAAA", "AC" * 3000, 2, 2)]               # list B of about 3,000 against a capacity of 88


def alphabet_cases():
    rng = _rng(ALPHABET)
    ref = rs(rng, 5000, hc.WIDE)
    seq = ""
    for j in range(12):                                                   # an extension ends at the first N and a copy seeds once: many short copies
        piece = ref[100 + 400 * j:400 + 400 * j]
        seq += (rc(piece) if j % 3 == 1 else piece) + "N" * (40 if j == 5 else 1 + j % 4)
    seq += rs(rng, 4000 - len(seq), hc.WIDE)
    return [Case(ALPHABET, ref, seq, 10, 30)]


def _copies(rng, ref, n, parts=4):
    """``n`` bases in ``parts`` mutated copies of stretches of ``ref``, forward and reverse-complemented in turn (so that both
    strands' entries hit all along x's list)."""
    h = n // parts
    out = ""
    for j in range(parts):
        length = h if j < parts - 1 else n - h * (parts - 1)
        at = 500 + j * ((len(ref) - 1000 - length) // (parts - 1))
        piece = mutate_every(rng, ref[at:at + length], 55 + 5 * (j % 2), 27 + j)
        out += rc(piece) if j % 2 else piece
    assert len(out) == n
    return out


def large_cases():
    rng = _rng(SIX_TILES)
    ref = rs(rng, 20000)
    out = [Case(SIX_TILES, ref, _copies(rng, ref, 12000), 10, 50)]
    rng = _rng(LONGEST)
    ref = rs(rng, 70000)
    out.append(Case(LONGEST, ref, _copies(rng, ref, LONG_MAX_X), 10, 50))
    rng = _rng(TOO_LONG)
    ref = rs(rng, 70000)
    out.append(Case(TOO_LONG, ref, _copies(rng, ref, LONG_MAX_X + 1), 10, 50))
    return out


_ALL = []


def all_cases():
    """Every case, in the fixture's order (generated once per process)."""
    if not _ALL:
        _ALL.extend([hc.by_name()[hc.TOO_LONG]] + edge_cases() + strand_cases() + one_y_cases() + chunk_cases() + overflow_cases()
                    + alphabet_cases() + large_cases())
        assert len({c.name for c in _ALL}) == len(_ALL)
    return list(_ALL)


def by_name():
    return {c.name: c for c in all_cases()}


def device_eligible(case):
    return 2 <= case.k <= 13 and len(case.seq) <= LONG_MAX_X


def load_expected():
    """name -> {"name", "k", "window", "crc", "segs"}: the reference's answers (tests/golden/make_hash_long_fixture.py)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hash_long.expected.json.gz")
    with gzip.open(path, "rb") as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


# ---- a sample whose reads carry pieces of more than 2,048 bases (--max_hash_len 5000) ----------------------------------------------
SAMPLE_CHROM, SAMPLE_LEN = "chrL", 40000
SAMPLE_INS, SAMPLE_INS2, SAMPLE_GAP = 3000, 2500, 2500


def sample_table():
    """-> (AlignmentTable with read bases, {chrom: sequence}): a 40 kb contig; 6 reads aligned 2000M 3000I 2000M near 10 kb whose
    insertion copies 1,500 bases of the reference under the alignment forwards and 1,500 reverse-complemented (one substitution
    every 97 bases), 6 reads aligned 1800M 2500I 2100M near 31 kb whose insertion is a reverse-complemented copy, and 6 reads split
    into 3000M at 20 kb and a supplementary 3000M at 26 kb with 2,500 unaligned bases (a copy of nearby reference) in between.
    The split reads' unaligned bases reach the re-aligner as EMPTY pieces: the collection keeps upstream's slicing of a segment's
    own bases with whole-read coordinates (analyze_reads._hash_between), so only the insertions are long jobs."""
    from svision_amd.io import bam
    rng = _rng("l/sample")
    ref = rs(rng, SAMPLE_LEN)
    recs = []                                                              # (pos, flag, name, cigar words, read)
    for j in range(6):
        r0 = 10000 + 40 * j
        h = SAMPLE_INS // 2
        ins = mutate_every(rng, ref[r0 + 400:r0 + 400 + h], 97, 11 + j) + rc(mutate_every(rng, ref[r0 + 2200:r0 + 2200 + h], 97, 11 + j))
        read = ref[r0:r0 + 2000] + ins + ref[r0 + 2000:r0 + 4000]
        recs.append((r0, 0, "ins%d" % j, [2000 << 4, SAMPLE_INS << 4 | 1, 2000 << 4], read))
    for j in range(6):                                                     # a second long shape through the collection
        r0 = 31000 + 35 * j
        ins = rc(mutate_every(rng, ref[r0 + 600:r0 + 600 + SAMPLE_INS2], 83, 5 + j))
        read = ref[r0:r0 + 1800] + ins + ref[r0 + 1800:r0 + 3900]
        recs.append((r0, 0, "inv%d" % j, [1800 << 4, SAMPLE_INS2 << 4 | 1, 2100 << 4], read))
    for j in range(6):
        r0, r1 = 20000 + 30 * j, 26000 + 30 * j
        gap = mutate_every(rng, ref[r0 + 3200:r0 + 3200 + SAMPLE_GAP], 89, 7 + j)
        read = ref[r0:r0 + 3000] + gap + ref[r1:r1 + 3000]
        recs.append((r0, 0, "split%d" % j, [3000 << 4, (SAMPLE_GAP + 3000) << 4 | 4], read))
        recs.append((r1, 2048, "split%d" % j, [(3000 + SAMPLE_GAP) << 4 | 4, 3000 << 4], read))
    recs.sort(key=lambda r: r[0])
    names, name_id, cigar, cig_off, packed, seq_off = [], [], [], [0], [], []
    at = 0
    for _pos, _flag, name, words, read in recs:
        if name not in names:
            names.append(name)
        name_id.append(names.index(name))
        cigar += words
        cig_off.append(len(cigar))
        raw = bam.pack_sequence(read)
        seq_off.append(at)
        packed.append(raw)
        at += len(raw)
    import numpy as np
    n = len(recs)
    table = bam.AlignmentTable([SAMPLE_CHROM], [SAMPLE_LEN], [0] * n, [r[0] for r in recs], [r[1] for r in recs], [60] * n,
                               [len(r[4]) for r in recs], name_id, names, np.array(cigar, np.uint32), cig_off,
                               "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n" % (SAMPLE_CHROM, SAMPLE_LEN),
                               seq_packed=np.frombuffer(b"".join(packed), np.uint8), seq_off=np.array(seq_off, np.int64))
    return table, {SAMPLE_CHROM: ref}
