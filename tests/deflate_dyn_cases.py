"""What the dynamic form of the BGZF encoder (svx_bgzf_deflate_dyn, csrc/svx_deflate_core.hpp encode_block_dyn) adds to
tests/deflate_enc_cases.py, shared by the host model's test (tests/test_bgzf_deflate_dyn_cpu.py) and the device's
(tests/test_gpu_bgzf_deflate_dyn.py): the crafted blocks that reach the code construction's corners, an own decoder of ONE final
dynamic block written against RFC 1951 (3.2.7) -- bit by bit, numpy and struct only --, the checks every member owes its input, and
the two host programs (tools/hostwave/deflate_dyn_main.cpp, and deflate_main.cpp for the fixed form's members)."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np

from tests import deflate_enc_cases as dc

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIB = [1, 1]
while len(FIB) < 22:
    FIB.append(FIB[-1] + FIB[-2])                               # 22 counts that add up to 46,367: Huffman's tree over them is 21 deep
FIB_BYTES = sum(FIB)
FIB_TAIL, FIB_EVEN = 16, 100                                    # fibonacci_tail_block: the counts 1, 2, 3 .. 1,597, and the values that share the rest
SMALL_SETS = ("collect_small", "ont_small")                     # the first FIRST blocks of these, every block of the other sets
FIRST = 8
SETS = ("collect_small", "ont_small", "straddling", "long", "decoy")


# ---- crafted blocks
def de_bruijn(k, n):
    """The de Bruijn sequence B(k, n) as a list of 0 .. k - 1, its first n - 1 entries appended: every n-gram exactly once."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq + seq[:n - 1]


def fibonacci_block(seed, values):
    """46,367 bytes: values[i] FIB[i] times, shuffled.  Huffman's tree over the BYTES is 21 deep, but the encoder codes tokens: the
    six values that make up 90 % of the block repeat their trigrams all over it, the parse turns nine bytes in ten into matches
    (about 1,300 literals and 13,300 matches a block), and the code over those tokens is 13 bits deep -- the limit is not reached."""
    buf = np.repeat(np.asarray(values, np.uint8), FIB)
    np.random.default_rng(seed).shuffle(buf)
    return buf.tobytes()


def fibonacci_tail_block(seed, values):
    """46,367 bytes: the counts 1, 2, 3, 5 .. 1,597 for the first FIB_TAIL values (the end-of-block symbol is the other 1 of the
    series), the rest of the block drawn evenly from FIB_EVEN other values, some 420 of each; shuffled, and then every byte that
    would complete a trigram a second time changes places with a later one: no trigram repeats, the parse finds no match (a match
    adds length symbols of small counts, which shorten the chain), every byte is a literal and the Fibonacci counts reach the code
    construction as they are.  The counts below 420 hang as a chain a dozen levels long under a subtree that weighs what one of the
    even values does, seven levels down: Huffman's tree over the tokens is deeper than 15 (check_member measures it)."""
    values = np.asarray(values, np.uint8)
    rng = np.random.default_rng(seed)
    tail = FIB[1:FIB_TAIL + 1]
    buf = np.concatenate([np.repeat(values[:FIB_TAIL], tail), rng.choice(values[FIB_TAIL:FIB_TAIL + FIB_EVEN], FIB_BYTES - sum(tail))])
    rng.shuffle(buf)
    buf, seen = buf.tolist(), set()
    for i in range(2, len(buf)):
        for _try in range(64):
            if (buf[i - 2], buf[i - 1], buf[i]) not in seen or i + 1 >= len(buf):
                break
            j = int(rng.integers(i + 1, len(buf)))
            buf[i], buf[j] = buf[j], buf[i]
        seen.add((buf[i - 2], buf[i - 1], buf[i]))
    return bytes(buf)


def huffman_depth(hist):
    """The depth of Huffman's tree over the counts {symbol: count} without any limit."""
    import heapq
    heap = [(n, 0) for n in hist.values() if n]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def all_literals_block():
    """Every byte value, and behind them -- every piece padded to a multiple of 64 bytes, so that a piece's positions keep their place
    in their wave -- the planted repeat of every length of deflate_enc_cases.LENGTHS at distance PLANT_DIST and of every distance of
    deflate_enc_cases.DISTANCES up to 2,049.  -> (bytes, [(length or None, distance)] planted)."""
    rng = np.random.default_rng(77)
    parts, want = [rng.permutation(256).astype(np.uint8).tobytes(), rng.permutation(256).astype(np.uint8).tobytes()], []
    plan = [(length, dc.PLANT_DIST, 100 + length, (length, dc.PLANT_DIST)) for length in dc.LENGTHS]
    plan += [(dc.PLANT_LEN, dist, 1000 + dist, (None, dist)) for dist in dc.DISTANCES if dist <= 2049]
    for length, dist, seed, token in plan:
        data, _at = dc.planted(length, dist, seed)
        parts.append(data + bytes(rng.integers(0, 144, -len(data) % 64, dtype=np.uint8)))
        want.append(token)
    out = b"".join(parts)
    assert len(out) <= dc.BLOCK
    return out, want


class DynCase(dc.Case):
    """A deflate_enc_cases.Case and: ``btype`` the block type the member must have (None: any), ``want_tokens`` matches it must hold,
    ``want_15`` a literal/length code of 15 bits where Huffman's tree over the tokens is deeper, ``dist_lens`` the distance code's lengths as the header gives them."""
    def __init__(self, name, data, btype=None, want_tokens=(), want_15=False, dist_lens=None, **kw):
        dc.Case.__init__(self, name, data, **kw)
        self.btype, self.want_tokens, self.want_15, self.dist_lens = btype, list(want_tokens), want_15, dist_lens


def crafted():
    """-> [DynCase]: the cases the dynamic form adds (the shared ones are deflate_enc_cases.crafted())."""
    rng = np.random.default_rng(12)
    out = [DynCase("distinct_bytes_no_match", rng.permutation(256)[:200].astype(np.uint8).tobytes())]
    # every trigram over 6 values exactly once: 218 literals of 2.6 bits of entropy and no match -- dynamic wins, nothing to code a distance with
    walk = bytes(65 + v for v in de_bruijn(6, 3))
    out.append(DynCase("no_match_six_values", walk, btype=2, dist_lens=[1, 1], no_long_match=True))
    # the same with ONE run in it: a literal and a match at distance 1, the only distance code there is
    out.append(DynCase("only_match_distance_1", walk[:100] + b"Z" * 30 + walk[100:], btype=2, want_tokens=[(29, 1)], dist_lens=[1, 1]))
    for k, lo in enumerate((0, 100, 234)):
        out.append(DynCase("fibonacci_bytes_%d" % k, fibonacci_block(30 + k, rng.permutation(22) + lo), btype=2))
        out.append(DynCase("fibonacci_%d" % k, fibonacci_tail_block(40 + k, rng.permutation(256)), btype=2, want_15=True))
    data, want = all_literals_block()
    out.append(DynCase("all_literals_and_planted", data, btype=2, want_tokens=want))
    tiny = bytearray(rng.integers(0, 144, 300, dtype=np.uint8).tobytes())
    tiny[200:240] = tiny[150:190]
    out.append(DynCase("tiny_300", bytes(tiny), btype=1))                    # a table costs more than it saves here
    return out


def all_cases():
    """The shared crafted cases and the dynamic form's -> [Case]."""
    return dc.crafted() + crafted()


def file_sets(tmp_dir):
    """-> [(set name, [block])] in the order of SETS: every block of straddling, long and decoy, the first eight of the two golden files."""
    by = {}
    for name, block in dc.bam_blocks(tmp_dir):
        by.setdefault(name.split("[")[0], []).append(block)
    return [(s, by[s][:FIRST] if s in SMALL_SETS else by[s]) for s in SETS]


# ---- the decoder
class Dynamic:
    """One final dynamic block, decoded: hlit, hdist, hclen as counts (257 .., 1 .., 4 ..), cl_lens [19] by symbol, lit_lens [hlit],
    dist_lens [hdist], and with ``tokens=True`` matches [(length, distance)], literals, lit_hist {literal/length symbol: count}."""


def _codes(lens):
    """Code lengths -> {(length, code): symbol} of the canonical code (RFC 1951, 3.2.2)."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    table = {}
    for sym, l in enumerate(lens):
        if l:
            table[(l, nxt[l])] = sym
            nxt[l] += 1
    return table


def kraft(lens):
    """The Kraft sum of a code's lengths in units of 2^-15: a complete code has 32,768."""
    return sum(1 << (15 - l) for l in lens if l)


def decode_dynamic(payload, tokens=True):
    bits = np.unpackbits(np.frombuffer(payload, np.uint8), bitorder="little").tolist()
    p = 0

    def take(n):                                                # a field: least significant bit first
        nonlocal p
        v = 0
        for i in range(n):
            v |= bits[p + i] << i
        p += n
        return v

    def symbol(table):                                          # a Huffman code: most significant bit first
        nonlocal p
        v = 0
        for l in range(1, 16):
            v = v << 1 | bits[p]
            p += 1
            if (l, v) in table:
                return table[(l, v)]
        raise AssertionError("no code of 15 bits or fewer")

    assert take(1) == 1 and take(2) == 2                        # BFINAL, BTYPE 10
    d = Dynamic()
    d.hlit, d.hdist, d.hclen = take(5) + 257, take(5) + 1, take(4) + 4
    assert d.hlit <= 286 and d.hdist <= 30
    d.cl_lens = [0] * 19
    for k in range(d.hclen):
        d.cl_lens[CL_ORDER[k]] = take(3)
    cl = _codes(d.cl_lens)
    lens = []
    while len(lens) < d.hlit + d.hdist:
        s = symbol(cl)
        if s < 16:
            lens.append(s)
        elif s == 16:
            assert lens
            lens += [lens[-1]] * (3 + take(2))
        elif s == 17:
            lens += [0] * (3 + take(3))
        else:
            lens += [0] * (11 + take(7))
    assert len(lens) == d.hlit + d.hdist
    d.lit_lens, d.dist_lens = lens[:d.hlit], lens[d.hlit:]
    d.matches, d.literals, d.lit_hist = [], 0, {256: 1}
    if tokens:
        lit, dist = _codes(d.lit_lens), _codes(d.dist_lens)
        while True:
            s = symbol(lit)
            if s == 256:
                break
            d.lit_hist[s] = d.lit_hist.get(s, 0) + 1
            if s < 256:
                d.literals += 1
                continue
            length = dc.LEN_BASE[s - 257] + take(dc.LEN_EXTRA[s - 257])
            ds = symbol(dist)
            d.matches.append((length, dc.DIST_BASE[ds] + take(dc.DIST_EXTRA[ds])))
        assert len(payload) == (p + 7) // 8
    return d


def check_header(d, name):
    """What every dynamic header owes RFC 1951 and the next decoder: three complete codes within their limits, nothing trimmed short."""
    assert max(d.lit_lens) <= 15 and max(d.dist_lens) <= 15 and max(d.cl_lens) <= 7, name
    assert kraft(d.lit_lens) == 32768 and kraft(d.dist_lens) == 32768 and kraft(d.cl_lens) == 32768, (name, kraft(d.lit_lens), kraft(d.dist_lens), kraft(d.cl_lens))
    for lens in (d.lit_lens, d.dist_lens, d.cl_lens):
        assert sum(1 for l in lens if l) >= 2, name
    assert d.lit_lens[256] > 0, name
    assert d.hlit == 257 or d.lit_lens[-1] != 0, name            # no trailing zero length is counted
    assert d.hdist == 1 or d.dist_lens[-1] != 0, name
    assert d.hclen == 4 or d.cl_lens[CL_ORDER[d.hclen - 1]] != 0, name


def check_member(member, data, btype, fixed_member, case=None, tokens=False):
    """deflate_enc_cases.check_member's checks with the block type 0, 1 or 2 and equal to ``btype``; never longer than the fixed
    program's member, and that member where the type is 0 or 1; a dynamic header by check_header.  ``tokens``: decode the token
    stream too (the crafted cases).  -> the decoded Dynamic, or None."""
    name = case.name if case is not None else "block"
    assert member[:16] == dc.HEADER, name
    assert struct.unpack_from("<H", member, 16)[0] + 1 == len(member) <= 65536, name
    payload = member[18:-8]
    assert zlib.decompress(payload, -15) == data, name
    z = zlib.decompressobj(-15)
    z.decompress(payload)
    assert z.eof and z.unused_data == b"", name
    assert struct.unpack_from("<II", member, len(member) - 8) == (zlib.crc32(data) & 0xFFFFFFFF, len(data)), name
    assert len(member) <= len(data) + 31, name
    assert payload[0] & 1 == 1 and (payload[0] >> 1) & 3 == btype and btype in (0, 1, 2), name      # one FINAL block
    assert len(member) <= len(fixed_member), name
    if btype == 0:
        assert len(member) == len(data) + 31, name
    if btype in (0, 1):
        assert member == fixed_member, name
        matches = dc.tokens(payload)[0] if btype == 1 and tokens else []
        d = None
    else:
        assert len(member) < len(fixed_member), name             # at a tie the older form wins
        d = decode_dynamic(payload, tokens)
        check_header(d, name)
        matches = d.matches
    if case is not None:
        if case.stored is not None:
            assert (btype == 0) == case.stored, name
        if case.max_member is not None:
            assert len(member) <= case.max_member, (name, len(member))
        if getattr(case, "btype", None) is not None:
            assert btype == case.btype, (name, btype)
        if tokens and btype != 0:
            assert all(3 <= l <= 258 and 1 <= dd <= 32768 for l, dd in matches), name
            want = list(getattr(case, "want_tokens", [])) + ([case.want_token] if case.want_token is not None else [])
            for wl, wd in want:
                assert any((wl is None or l == wl) and (wd is None or dd == wd) for l, dd in matches), (name, wl, wd)
            if case.no_long_match:
                assert not any(l >= 8 for l, _dd in matches), name
        if d is not None and getattr(case, "want_15", False):
            assert max(d.lit_lens) == 15 and (not tokens or huffman_depth(d.lit_hist) > 15), name
        if d is not None and getattr(case, "dist_lens", None) is not None:
            assert d.dist_lens == case.dist_lens, (name, d.dist_lens)
    return d


def zlib_members(blocks, level):
    """The bytes zlib at ``level`` (default strategy) writes for the blocks as BGZF members: 26 bytes of header and footer a block."""
    total = 0
    for b in blocks:
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(co.compress(b)) + len(co.flush()) + 26
    return total


# ---- the host programs
def build_host(tmp_dir, source, sanitize=False):
    """tools/hostwave/<source>.cpp as a stand-alone program -> its path; ``sanitize``: under AddressSanitizer and UBSan."""
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_dir / (source + ("_san" if sanitize else "")))
    checks = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O2"] + checks + ["-o", out, os.path.join(dc.ROOT, "tools", "hostwave", source + ".cpp"), "-lz"])
    return out


def run_host(program, tmp_dir, tag, case_blocks, file_blocks, case_orders, file_orders):
    """A host program on the crafted blocks in ``case_orders`` thread orders and on the files' blocks in ``file_orders``, the latter
    shared out to deflate_enc_cases.PARTS processes that run side by side -> per order (members, flags: the stored flag or the block
    type), crafted blocks first, then the files' blocks where that order ran on them."""
    jobs = [(tag + "cases", case_blocks, case_orders)] + [("%sfiles%d" % (tag, k), file_blocks[k::dc.PARTS], file_orders) for k in range(dc.PARTS)]
    procs = []
    for name, blocks, orders in jobs:
        dc.write_cases(str(tmp_dir / (name + ".bin")), blocks)
        procs.append(subprocess.Popen([program, str(tmp_dir / (name + ".bin")), str(tmp_dir / name), str(orders)], stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    for p in procs:
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0 and "FAILED" not in out and "host: ok" in out, out[-3000:] + err[-3000:]
    per_order = []
    for o in range(case_orders):
        got, flags = dc.read_members(str(tmp_dir / ("%scases.%d" % (tag, o))))
        if o < file_orders:
            got_f, flags_f = [None] * len(file_blocks), [None] * len(file_blocks)
            for k in range(dc.PARTS):
                got_f[k::dc.PARTS], flags_f[k::dc.PARTS] = dc.read_members(str(tmp_dir / ("%sfiles%d.%d" % (tag, k, o))))
            got, flags = got + got_f, flags + flags_f
        per_order.append((got, flags))
    return per_order
