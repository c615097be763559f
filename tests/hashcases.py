"""The catalogue of --hash re-aligner cases beyond k = 10, window = 50 and 900 bases, from fixed seeds: shared by the
script that records the reference's answers (tests/golden/make_hash_params_fixture.py), the CPU test of the host aligner
(tests/test_hash_params_cpu.py) and the GPU tests of svx_hash_seeds (tests/test_gpu_hash_seeds.py).

A case: ``(name, ref, seq, k, window)`` -- ``ref`` the reference window (y), ``seq`` the piece to place (x).  The name starts
with the group: ``a`` parameter sweep, ``b`` tiny k, ``c`` full table, ``d`` chunk boundaries, ``e`` list order at one y
position, ``f`` large window, ``g`` degenerate, ``k14`` k above the kernel's limit.  Every sequence is a function of the
case's name alone, so the fixture stores names and results, not bases.

``raw_hit_lists`` is the host aligner's two hit lists before the filter and the merge, in the device's record form."""
import collections
import gzip
import json
import os
import random
import zlib

Case = collections.namedtuple("Case", "name ref seq k window")

WIDE = "ACGT" * 8 + "NacgtnRYKMS"              # mostly upper-case ACGT plus every other symbol pack_bases admits
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}

SWEEP = [(7, 30), (10, 10), (10, 120), (12, 30), (13, 13), (13, 50)]
SHAPES = ["fwd", "rc", "mix", "novel"]
SWEEP_PER_PARAM = 12                            # 3 of each shape; every third case draws from WIDE
TINY = [(2, 2), (2, 50), (3, 3), (3, 20)]
FULL_LENS = [2048, 2047, 2040]
FULL_PARAMS = [(2, 2), (10, 50), (13, 50)]
MAX_X = 2048                                    # the device kernel's longest piece
OVERFLOW = "b/overflow/k2w2"
ALL_AVOIDED = ["b/avoided/k2w2/3000", "b/avoided/k3w3/500"]
TOO_LONG = "c/piece2049/k10w50"
CHUNKS = "d/mutated/k10w50"
CHUNK_EDGE = "d/y255-257/k10w50"
ONE_Y = "e/one-y/k10w50"
LARGE = "f/window20000/k10w50"


def _rng(name):
    return random.Random(zlib.crc32(name.encode()))


def rs(rng, n, alphabet="ACGT"):
    return "".join(rng.choices(alphabet, k=n))


def rc(s):
    """Reverse complement as the aligner sees it: anything but upper-case ACGT becomes N."""
    return "".join(_COMP.get(c, "N") for c in reversed(s))


def other(rng, base):
    return rng.choice([c for c in "ACGT" if c != base])


def mutate_every(rng, s, step, first):
    """Substitute the bases first, first + step, ... of ``s``."""
    s = list(s)
    for p in range(first, len(s), step):
        s[p] = other(rng, s[p])
    return "".join(s)


# ---- a: parameter sweep -----------------------------------------------------------------------------------------------------
def _sweep(k, window, n):
    shape = SHAPES[n % 4]
    name = "a/k%dw%d/%02d-%s" % (k, window, n, shape)
    rng = _rng(name)
    alphabet = WIDE if n % 3 == 2 else "ACGT"
    ylen = rng.randint(max(60, min(1500, 2 * window + 40)), 1500)      # long enough to hold a copy of `window` bases
    ref = rs(rng, ylen, alphabet)
    lo = min(ylen, window + 12)
    length = rng.randint(lo, min(ylen, max(lo, 900)))
    at = rng.randrange(0, ylen - length + 1)
    copy = ref[at:at + length]
    if shape == "fwd":
        seq = copy
    elif shape == "rc":
        seq = rc(copy)
    elif shape == "mix":
        seq = rs(rng, rng.randint(0, 80), alphabet) + copy + rs(rng, rng.randint(0, 80), alphabet) + rc(copy[:length // 2])
    else:
        seq = rs(rng, rng.randint(30, 900), alphabet)
    return Case(name, ref, seq, k, window)


def sweep_cases():
    return [_sweep(k, w, n) for k, w in SWEEP for n in range(SWEEP_PER_PARAM)]


def is_planted(case):
    return case.name.startswith("a/") and not case.name.endswith("-novel")


def sweep_group(case):
    return case.name.split("/")[1]


# ---- b: tiny k --------------------------------------------------------------------------------------------------------------
def tiny_cases():
    out = []
    # every k-mer of a long window occurs twice or more among its own k-mers: all avoided, no seed at all
    rng = _rng(ALL_AVOIDED[0])
    ref = rs(rng, 3000)
    out.append(Case(ALL_AVOIDED[0], ref, ref[700:1900], 2, 2))
    rng = _rng(ALL_AVOIDED[1])
    ref = rs(rng, 500)
    out.append(Case(ALL_AVOIDED[1], ref, ref[100:400], 3, 3))
    # hits at k = 2 / 3 need windows of a handful of distinct k-mers: "AC" (or "ACT") occurs once on either strand
    out.append(Case(OVERFLOW, "ACAAAA", "AC" * 1024, 2, 2))            # 1 A-hit, 1023 B-hits against a capacity of 4*6+64 = 88
    out.append(Case("b/hand/k2w2/repeat-under-cap", "ACAAAA", "AC" * 40, 2, 2))
    out.append(Case("b/hand/k2w2/both-strands", "ACAAAAA", "TTACAAAGGTTTGTCC", 2, 2))
    out.append(Case("b/hand/k2w2/wide", "RYAAAAAAn", "ccRYAAAAnnRYAAKMS", 2, 2))
    out.append(Case("b/hand/k2w50/run", "AC" + "G" * 70, "TAC" + "G" * 80 + "AC" + "G" * 60, 2, 50))
    out.append(Case("b/hand/k2w50/short-window", "AC" + "G" * 40, "AC" + "G" * 80, 2, 50))
    out.append(Case("b/hand/k3w3/both-strands", "ACTAAAAAA", "GGACTAAACCTTTAGTCC", 3, 3))
    out.append(Case("b/hand/k3w3/repeat", "CCCCACTCCCC", "ACT" * 30 + "CACTCC" + "AGTG" * 5, 3, 3))
    out.append(Case("b/hand/k3w20/run", "ACT" + "G" * 30, "CACT" + "G" * 25 + "TACT" + "G" * 40 + rc("ACT" + "G" * 28) + "A", 3, 20))
    out.append(Case("b/hand/k3w20/N-stops", "ACT" + "G" * 30, "ACT" + "G" * 12 + "N" + "G" * 30 + "ACT" + "G" * 22 + "NN", 3, 20))
    return out


# ---- c: full table ------------------------------------------------------------------------------------------------------------
def _three_copies(rng, ref, total):
    """fwd piece + 3 junk + rc piece + 5 junk + fwd piece, ``total`` bases, the pieces cut from ``ref``."""
    n = (total - 8) // 3
    last = total - 8 - 2 * n
    a, b, c = (rng.randrange(0, len(ref) - last) for _ in range(3))
    return ref[a:a + n] + rs(rng, 3) + rc(ref[b:b + n]) + rs(rng, 5) + ref[c:c + last]


def full_cases():
    out = []
    for total in FULL_LENS:
        for k, window in FULL_PARAMS:
            name = "c/piece%d/k%dw%d" % (total, k, window)
            rng = _rng(name)
            ref = rs(rng, 3000)
            out.append(Case(name, ref, _three_copies(rng, ref, total), k, window))
    rng = _rng(TOO_LONG)
    ref = rs(rng, 3000)
    out.append(Case(TOO_LONG, ref, _three_copies(rng, ref, MAX_X + 1), 10, 50))
    return out


# ---- d: chunk boundaries (the kernel walks y in chunks of 256 positions) -------------------------------------------------------
def chunk_cases():
    rng = _rng(CHUNKS)
    ref = rs(rng, 6000)
    seq = mutate_every(rng, ref[1000:2000], 60, 30) + rc(mutate_every(rng, ref[3000:4040], 55, 27))
    out = [Case(CHUNKS, ref, seq, 10, 50)]
    # three copies that start at y = 255, 256 and 257, each behind a base that differs from the window's previous one
    rng = _rng(CHUNK_EDGE)
    ref = rs(rng, 1500)
    seq = ref[255:315] + other(rng, ref[255]) + ref[256:316] + other(rng, ref[256]) + ref[257:317] + rs(rng, 4)
    out.append(Case(CHUNK_EDGE, ref, seq, 10, 50))
    return out


# ---- e: several hits at one y position, both strands ----------------------------------------------------------------------------
def order_cases():
    rng = _rng(ONE_Y)
    u = rs(rng, 70)
    ref = rs(rng, 300) + u + rs(rng, 300)
    seq = rs(rng, 7) + u + rs(rng, 9) + rc(u) + rs(rng, 11) + u + rs(rng, 5) + rc(u) + rs(rng, 3)
    return [Case(ONE_Y, ref, seq, 10, 50)]


# ---- f: large window ------------------------------------------------------------------------------------------------------------
def large_cases():
    rng = _rng(LARGE)
    ref = rs(rng, 20000)
    return [Case(LARGE, ref, ref[9000:11000], 10, 50)]


# ---- g: degenerate ------------------------------------------------------------------------------------------------------------
def degenerate_cases():
    rng = _rng("g")
    r = rs(rng, 500)
    n5 = "ACGT" * 19 + "N" * 4                                          # 5 % N
    pal = "ACGTACGT" + "TTAA" + "ACGTACGT"                             # its own reverse complement
    out = []
    for k, window in ((10, 50), (2, 2), (13, 13)):
        tag = "k%dw%d" % (k, window)
        out += [
            Case("g/empty-piece/" + tag, rs(rng, 300), "", k, window),
            Case("g/empty-window/" + tag, "", rs(rng, 300), k, window),
            Case("g/both-empty/" + tag, "", "", k, window),
            Case("g/both-short/" + tag, rs(rng, k + 1), rs(rng, k + 1), k, window),
            Case("g/short-piece/" + tag, rs(rng, 400), rs(rng, k - 1), k, window),
            Case("g/short-window/" + tag, rs(rng, k), rs(rng, 300), k, window),
            Case("g/k+2/" + tag, r[:k + 2], r[:k + 2], k, window),
            Case("g/equal/" + tag, r, r, k, window),
            Case("g/equal-rc/" + tag, r, rc(r), k, window),
            Case("g/palindrome-repeat/" + tag, rs(rng, 100) + pal * 6 + rs(rng, 100), pal * 4, k, window),
            Case("g/unit-repeat/" + tag, "ACGT" * 100, "ACGT" * 40, k, window),
            Case("g/N-runs/" + tag, rs(rng, 300, n5), rs(rng, 200, n5), k, window),
            Case("g/inner-copy/" + tag, r, r[100:350], k, window),
            Case("g/inner-rc/" + tag, r, rc(r[50:400]), k, window),
        ]
    return out


# ---- k above the device kernel's 13 (host path only) ------------------------------------------------------------------------------
def k14_cases():
    out = []
    for n in (0, 1, 2):
        c = _sweep(14, 50, n)
        out.append(Case("k14/%02d-%s" % (n, SHAPES[n % 4]), c.ref, c.seq, 14, 50))
    return out


_ALL = []


def all_cases():
    """Every case, in the fixture's order (generated once per process)."""
    if not _ALL:
        _ALL.extend(sweep_cases() + tiny_cases() + full_cases() + chunk_cases() + order_cases() + large_cases()
                    + degenerate_cases() + k14_cases())
        assert len({c.name for c in _ALL}) == len(_ALL)
    return list(_ALL)


def by_name():
    return {c.name: c for c in all_cases()}


def digest(case):
    """What the fixture keeps of a case's sequences: enough to notice that they were regenerated differently."""
    return zlib.crc32(("%s|%s|%d|%d" % (case.ref, case.seq, case.k, case.window)).encode())


def load_expected():
    """name -> {"name", "k", "window", "crc", "segs"}: the reference's answers (tests/golden/make_hash_params_fixture.py)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hash_params.expected.json.gz")
    with gzip.open(path, "rb") as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def device_eligible(case):
    """Cases the device kernel takes: 2 <= k <= 13 and a piece of at most MAX_X bases (all alphabets here pack)."""
    return 2 <= case.k <= 13 and len(case.seq) <= MAX_X


def fmt(segments):
    return [[s.xStart(), s.xEnd(), s.yStart(), s.yEnd(), bool(s.forward())] for s in segments]


# ---- the host aligner's raw lists -------------------------------------------------------------------------------------------------
def raw_hit_lists(ref, seq, k, window):
    """-> (hits_a, hits_b): the host aligner's hits of the self pass and of the placement pass, every one kept, in its
    loop order, as the device's records [y position, x position or position in x's reverse complement, match length,
    forward]."""
    from svision_amd.segmentplot.hash_aligner import HashAligner
    a = HashAligner(k, window, 0, 2)
    a.run(ref, ref)
    hits_a = [[s.yStart(), s.xStart() if s.forward() else (len(ref) - 1) - s.xStart(), s._length, int(bool(s.forward()))]
              for s in a.getSegments()]
    b = HashAligner(k, window, 0, 2)
    b.compareDiffSegs = []                                   # keep every hit
    b.y_hashvalues = a.getHashValues()
    b._align(seq, ref, a.getAvoidKmer())
    hits_b = [[s.yStart(), s.xStart() if s.forward() else (len(seq) - 1) - s.xStart(), s._length, int(bool(s.forward()))]
              for s in b.getSegments()]
    return hits_a, hits_b


_RAW = {}


def raw_hit_lists_of(case):
    """``raw_hit_lists`` of a catalogue case, computed once per process."""
    if case.name not in _RAW:
        _RAW[case.name] = raw_hit_lists(case.ref, case.seq, case.k, case.window)
    return _RAW[case.name]
