"""The catalogue of DEFLATE streams zlib never writes (tests/deflate_writer.py), as BGZF blocks, from fixed seeds: shared by
the CPU test that proves every case holds the construct it claims (test_deflate_writer_cpu.py) and the GPU test that runs
every device inflater on it (test_gpu_inflate_streams.py).

A case: name, group, the BGZF blocks [(bytes, intended output)] and a ``feature`` check on what ``deflate_writer.inspect``
finds in them.  The groups are launched one at a time: the "phase" and "slot" groups depend on where their blocks sit in
the launch (output phase mod 64, the fast path's sequence-stream slots)."""
import random
import struct

from tests import deflate_writer as dw

SEG_BITS, CHUNK_BITS = 512, 64 * 512        # the tokens kernel's lane segment and staged chunk (svx_inflate2.hip)


class Case:
    def __init__(self, name, group, members, feature):
        self.name, self.group, self.members, self.feature = name, group, members, feature


def payload(block):
    """A BGZF block -> its raw DEFLATE bytes (BC found among any subfields)."""
    xlen = struct.unpack_from("<H", block, 10)[0]
    bsize = None
    p = 12
    while p < 12 + xlen:
        slen = struct.unpack_from("<H", block, p + 2)[0]
        if block[p:p + 2] == b"BC":
            bsize = struct.unpack_from("<H", block, p + 4)[0]
        p += 4 + slen
    return block[12 + xlen:bsize + 1 - 8]


def _frame(d, extra=(), isize=None):
    return dw.bgzf(d.getvalue(), bytes(d.data), isize=isize, extra=extra), bytes(d.data)


def _rand(rng, n, alphabet=None):
    if alphabet is None:
        return bytes(rng.getrandbits(8) for _ in range(n))
    return bytes(rng.choice(alphabet) for _ in range(n))


def _length_range(li):
    lo = dw.LEN_BASE[li]
    return lo, (lo if li == 28 else lo + (1 << dw.LEN_EXTRA[li]) - 1)


def _dist_range(di):
    lo = dw.DIST_BASE[di]
    return lo, lo + (1 << dw.DIST_EXTRA[di]) - 1


def cover_tokens(rng, lit_lens, dist_lens, have, extra=200):
    """Tokens that use EVERY literal / length and distance symbol of nonzero length (at least once), shuffled, plus ``extra``
    random ones; ``have``: output bytes in front of them (matches never reach further)."""
    lits = [s for s in range(256) if lit_lens[s]]
    lcodes = [s - 257 for s in range(257, min(len(lit_lens), 286)) if lit_lens[s]]
    dcodes = [d for d in range(min(len(dist_lens), 30)) if dist_lens[d]]
    items = [("l", s) for s in lits] + [("m", li) for li in lcodes]
    if lcodes:
        items += [("d", di) for di in dcodes]
    items += [("r", None)] * extra
    rng.shuffle(items)
    out, n = [], have
    for kind, v in items:
        if kind == "l" or (kind == "r" and (not lcodes or rng.random() < 0.5)):
            out.append(v if kind == "l" else rng.choice(lits))
            n += 1
            continue
        li = v if kind == "m" else rng.choice(lcodes)
        ok = [d for d in dcodes if dw.DIST_BASE[d] <= n]
        if kind == "d":
            if v not in ok:
                raise ValueError("distance code %d needs more history" % v)
            di = v
        else:
            if not ok:
                out.append(rng.choice(lits))
                n += 1
                continue
            di = rng.choice(ok)
        length = rng.randint(*_length_range(li))
        dlo, dhi = _dist_range(di)
        out.append((length, rng.randint(dlo, min(dhi, n))))
        n += length
    return out


def _lengths(rng, n, used, skew=None):
    """A complete code over the symbols ``used`` of an alphabet of n: random (or Fibonacci-skewed) frequencies."""
    f = [0] * n
    order = list(used)
    rng.shuffle(order)
    fib = [1, 1]
    while len(fib) < len(order):
        fib.append(fib[-1] + fib[-2])
    for k, s in enumerate(order):
        f[s] = fib[len(order) - 1 - k] if skew == "fib" else rng.randint(1, 1000)
    return dw.huffman_lengths(f)


def _swap_to(lens, idx, value, avoid=()):
    """Permute the lengths of one alphabet (still the same code) so that lens[i] == value for i in idx, != value at avoid."""
    lens = list(lens)
    for i in idx:
        if lens[i] != value:
            j = next(j for j in range(len(lens)) if lens[j] == value and j not in idx and j not in avoid)
            lens[i], lens[j] = lens[j], lens[i]
    for i in avoid:
        if lens[i] == value:
            j = next(j for j in range(len(lens)) if lens[j] not in (value, 0) and j not in idx and j not in avoid)
            lens[i], lens[j] = lens[j], lens[i]
    return lens


def _fit_literals(bits):
    """(a, b): a literals of 8 bits and b of 9 bits in the fixed code fill exactly ``bits`` bits (bits >= 56)."""
    b = bits % 8
    a = (bits - 9 * b) // 8
    assert a >= 0 and 8 * a + 9 * b == bits, bits
    return a, b


def _fixed_of_bits(rng, body_bits, matches=True, have=0):
    """Fixed-code tokens whose codes + the EOB take exactly ``body_bits`` bits: random tokens (literals, short matches), then
    8- and 9-bit literals for the rest."""
    toks, used, n = [], 0, have
    while body_bits - used > 200:
        if matches and n >= 16 and rng.random() < 0.3:
            length, dist = rng.randint(3, 10), rng.randint(1, 16)
            toks.append((length, dist))              # codes 257..264 (7 bits) + distance codes 0..7 (5 + 0..2 bits)
            used += 7 + 5 + dw.DIST_EXTRA[dw.dist_code(dist)]
            n += length
        else:
            c = rng.getrandbits(8)
            toks.append(c)
            used += 8 if c < 144 else 9
            n += 1
    a, b = _fit_literals(body_bits - used - 7)
    toks += [rng.randrange(0, 144) for _ in range(a)] + [rng.randrange(144, 256) for _ in range(b)]
    return toks


def _stream_size(blocks):
    """The tokens kernel's sequence stream (bytes, not counting the SPLIT pad) for a DEFLATE stream of dynamic / fixed blocks
    whose tokens each fit one lane segment and contain no match, and stored blocks."""
    z = 0
    for b in blocks:
        n = b.out1 - b.out0
        if b.btype == 0:
            z += n + 4 * ((n + 254) // 255)
        else:
            assert not b.matches and b.end - b.body <= SEG_BITS and n <= 255
            z += 4 + n if n else 0
    return z


def slot_layout(isizes):
    """Per block of a launch: (slot bytes, pad of the SPLIT form) -- stream_base() of svx_inflate2.hip (the workspace's stream area
    starts 16-byte aligned)."""
    d = [0]
    for x in isizes:
        d.append(d[-1] + x)
    base = [d[b] + (d[b] >> 1) + 1024 * b for b in range(len(isizes) + 1)]
    head = (8 * len(isizes) + 255) & ~255
    return [(base[b + 1] - base[b], (-(head + base[b])) & 3) for b in range(len(isizes))]


# ---------------------------------------------------------------------------------------------------------------------

def build(seed=20261016):
    rng = random.Random(seed)
    cases = []

    def add(name, group, members, feature):
        cases.append(Case(name, group, members, feature))

    # ---- A. Huffman tables and headers
    # 18 across HLIT: lengths 280..285 unused (HLIT 286) and distance codes 0..9 unused; HDIST 30 with trailing zeros
    for mode in ("combined", "max-runs"):
        lit = _lengths(rng, 286, list(range(257)) + list(range(257, 280)))
        dist = _lengths(rng, 30, range(10, 16))
        d = dw.Deflate()
        d.stored(_rand(rng, 300))
        d.dynamic(cover_tokens(rng, lit, dist, 300), lit_lens=lit, dist_lens=dist, header=mode, hlit=286, hdist=30, final=True)
        add("cross18_" + mode, "A", [_frame(d)],
            lambda r: any(s == 18 for s, _a, _n in dw.crossing_runs(r[0][0][1])) and r[0][0][1].hlit == 286 and r[0][0][1].hdist == 30
            and r[0][0][1].dist_lens[-1] == 0)
    # 17 across HLIT: 282, 283 unused (HLIT 284), distance codes 0, 1 unused
    lit = _lengths(rng, 286, list(range(257)) + list(range(257, 282)))
    dist = _lengths(rng, 30, range(2, 12))
    d = dw.Deflate()
    d.stored(_rand(rng, 100))
    d.dynamic(cover_tokens(rng, lit, dist, 100), lit_lens=lit, dist_lens=dist, header="combined", hlit=284, final=True)
    add("cross17", "A", [_frame(d)], lambda r: any(s == 17 for s, _a, _n in dw.crossing_runs(r[0][0][1])))
    # 16 across HLIT, starting right AT HLIT (its previous length is the last literal / length one) and inside the distance
    # lengths; all 286 + 30 symbols in use, matches reach back into a stored block
    for start_at_hlit in (True, False):
        for _try in range(100):
            lit = _lengths(rng, 286, range(286))
            dist = _lengths(rng, 30, range(30), skew="fib" if _try % 2 else None)
            common = [v for v in set(dist) if dist.count(v) >= 4 and lit.count(v) >= 3]
            if common:
                break
        v = common[0]
        if start_at_hlit:
            lit = _swap_to(lit, [285], v, avoid=[284])
        else:
            lit = _swap_to(lit, [283, 284, 285], v, avoid=[282])
        dist = _swap_to(dist, [0, 1, 2, 3], v, avoid=[4])
        d = dw.Deflate()
        d.stored(_rand(rng, 32768))
        d.dynamic(cover_tokens(rng, lit, dist, 32768), lit_lens=lit, dist_lens=dist, header="combined", final=True)
        if start_at_hlit:
            add("cross16_at_hlit", "A", [_frame(d)],
                lambda r: any(s == 16 and at == r[0][0][1].hlit for s, _x, at in r[0][0][1].runs)
                and len(r[0][0][1].lit_syms) == 286 and len(r[0][0][1].dist_syms) == 30)
        else:
            add("cross16_all_symbols", "A", [_frame(d)],
                lambda r: any(s == 16 for s, _a, _n in dw.crossing_runs(r[0][0][1])) and r[0][0][1].hlit == 286
                and len(r[0][0][1].lit_syms) == 286 and len(r[0][0][1].dist_syms) == 30)
    # 16 repeating a zero, 18 x 138, 17 x 3, 16 x 6 (max-runs); HCLEN minimal and 19 with trailing zeros
    for hclen in ("min", "full"):
        lit = _lengths(rng, 286, [0, 11, 18, 25, 32, 39, 46] + list(range(200, 257)) + [257, 258, 270])
        dist = _lengths(rng, 30, [0, 3, 9, 29])
        d = dw.Deflate()
        d.stored(_rand(rng, 25000))
        d.dynamic(cover_tokens(rng, lit, dist, 25000), lit_lens=lit, dist_lens=dist, header="max-runs", hclen=hclen, final=True)

        def f(r, hclen=hclen):
            b = r[0][0][1]
            runs = [(s, x) for s, x, _at in b.runs]
            zero16 = any(s == 16 and b.runs[k - 1][0] in (0, 17, 18) for k, (s, _x, _at) in enumerate(b.runs) if k)
            last = max(k for k in range(19) if b.cl_lens[dw.CLEN_ORDER[k]]) + 1
            want = (b.hclen == 19 and b.cl_lens[dw.CLEN_ORDER[18]] == 0) if hclen == "full" else b.hclen == max(4, last) < 19
            return (18, 127) in runs and (17, 0) in runs and (16, 3) in runs and zero16 and want
        add("maxruns_hclen_" + hclen, "A", [_frame(d)], f)
    # HLIT 257 (literals only) with HDIST 1 of length 0; HDIST 1 with a single distance code of length 1
    d = dw.Deflate()
    d.dynamic(list(_rand(rng, 3000, b"ACGTN")), final=True, header="zlib")
    add("hlit257_hdist1_len0", "A", [_frame(d)], lambda r: r[0][0][0].hlit == 257 and r[0][0][0].hdist == 1 and r[0][0][0].dist_lens == [0])
    toks = [65] + [(rng.randint(3, 258), 1) if k % 2 else rng.randrange(256) for k in range(400)]
    for mode in ("zlib", "combined", "plain"):
        d = dw.Deflate()
        d.dynamic(toks, final=True, header=mode)
        add("single_distance_code_" + mode, "A", [_frame(d)], lambda r: r[0][0][0].hdist == 1 and r[0][0][0].dist_lens == [1] and r[0][0][0].matches)
    # an end-of-block-only dynamic block in front of data; 15-bit literal / length and distance codes (Fibonacci-skewed): past
    # every root table, the longest code (all ones) under the last root prefix
    for k in range(3):
        lit = _lengths(rng, 286, range(286), skew="fib")
        dist = _lengths(rng, 30, range(30), skew="fib")
        d = dw.Deflate()
        d.dynamic([], header=("zlib", "plain", "combined")[k])
        d.stored(_rand(rng, 32768))
        d.dynamic(cover_tokens(rng, lit, dist, 32768, extra=100), lit_lens=lit, dist_lens=dist, header=("zlib", "combined", "max-runs")[k], final=True)

        def f(r):
            e, _s, b = r[0][0]
            ok = e.btype == 2 and e.out1 == e.out0 and not e.lit_syms - {256}
            for lens, syms in ((b.lit_lens, b.lit_syms), (b.dist_lens, b.dist_syms)):
                codes = dw.canonical(lens)
                top = [s for s in syms if lens[s] == 15 and codes[s] == 0x7FFF]
                ok = ok and max(lens) == 15 and dw.kraft(lens) == 1 << 15 and top
            return ok
        add("fib15_%d" % k, "A", [_frame(d)], f)
    # fixed blocks with lengths 115..258 (codes 280..285) and distance code 29
    d = dw.Deflate()
    d.stored(_rand(rng, 30000))
    toks = []
    for li in range(23, 29):
        for _ in range(3):
            toks += [rng.randrange(256), (rng.randint(*_length_range(li)), rng.randint(24577, 30000))]
    d.fixed(toks, final=True)
    add("fixed_long_far", "A", [_frame(d)],
        lambda r: set(range(280, 286)) <= r[0][0][1].lit_syms and 29 in r[0][0][1].dist_syms and r[0][0][1].btype == 1)

    # ---- B. Block structure inside one BGZF block
    text = _rand(rng, 20000, b"ACGTTGCAAC")
    d = dw.Deflate()
    d.fixed(dw.greedy_lz77(text[:4000]))
    d.stored(b"")
    d.dynamic(dw.greedy_lz77(text[4000:10000], history=text[:4000]), header="zlib")
    d.dynamic(dw.greedy_lz77(text[10000:16000], history=text[:10000]), header="combined")
    d.stored(text[16000:], final=True)
    add("mixed_sequence", "B", [_frame(d)], lambda r: [b.btype for b in r[0][0]] == [1, 0, 2, 2, 0] and r[0][0][1].len == 0)
    # stored headers at every bit phase
    d = dw.Deflate()
    for p in range(8):
        for n9 in range(8):
            if (d.w.pos + 3 + 8 + 9 * n9 + 7) % 8 == p:
                break
        d.fixed([rng.randrange(144)] + [rng.randrange(144, 256) for _ in range(n9)])
        d.stored(_rand(rng, rng.randint(0, 40)))
    d.stored(b"end", final=True)
    add("stored_every_phase", "B", [_frame(d)], lambda r: {b.start % 8 for b in r[0][0] if b.btype == 0} == set(range(8)))
    # matches that reach back across DEFLATE blocks into stored and fixed data, up to 32,768
    far = _rand(rng, 20000)
    mid = _rand(rng, 13000)
    d = dw.Deflate()
    d.stored(far)
    d.fixed(list(mid))
    toks = [(258, 32768), (3, 32768 - 1), (100, 20000), (50, 13000), (258, 12999)]
    toks += [(rng.randint(3, 258), rng.randint(1, 32768)) for _ in range(150)]
    d.dynamic(toks, header="combined", final=True)
    add("matches_across_blocks", "B", [_frame(d)],
        lambda r: max(m[2] for m in r[0][0][2].matches) == 32768 and any(m[0] - m[2] < r[0][0][1].out0 for m in r[0][0][2].matches)
        and any(r[0][0][1].out0 <= m[0] - m[2] < r[0][0][2].out0 for m in r[0][0][2].matches))
    # EOB at / one bit before / one bit after a segment edge and the chunk edge (from the end of the block's header)
    targets = [e + k for e in (SEG_BITS, 7 * SEG_BITS, 63 * SEG_BITS, CHUNK_BITS) for k in (-1, 0, 1)]
    d = dw.Deflate()
    for t in targets:
        d.fixed(_fixed_of_bits(rng, t, have=len(d.data)))
    d.stored(b"", final=True)
    add("eob_at_edges", "B", [_frame(d)], lambda r: sorted(b.end - b.body for b in r[0][0] if b.btype == 1) == sorted(targets))
    # a dynamic header that straddles the chunk edge of the block in front
    d = dw.Deflate()
    d.fixed(_fixed_of_bits(rng, CHUNK_BITS - 40))
    d.dynamic(dw.greedy_lz77(text[:3000]), header="zlib", hclen="full", final=True)
    add("header_across_chunk_edge", "B", [_frame(d)],
        lambda r: r[0][0][1].start < r[0][0][0].body + CHUNK_BITS < r[0][0][1].body)

    # ---- C. LZ copies, explicit tokens
    dists = [1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 63, 64, 65, 239, 240, 241, 255, 256, 257, 4095, 4096, 4097, 32767, 32768]
    lens = list(range(3, 11)) + [15, 16, 17, 63, 64, 65, 255, 256, 257, 258]
    for k, dist in enumerate(dists):
        hist = _rand(rng, max(dist, 64))
        toks = [(258, dist)]                                   # first a match right behind the history
        for L in lens:
            toks += [rng.randrange(256) for _ in range(rng.randint(0, 3))] + [(L, dist)]
        toks.append((258, dist))                               # the block ends with a match
        d = dw.Deflate()
        if dist >= 256:
            d.stored(hist)
        else:
            d.fixed(list(hist))
        (d.fixed if k % 2 else d.dynamic)(toks, final=True)
        add("lz_d%d" % dist, "C", [_frame(d)],
            lambda r, dist=dist: {(m[1], m[2]) for m in r[0][0][1].matches} >= {(L, dist) for L in lens} and r[0][0][1].matches[-1][0] + 258 == r[0][0][1].out1)
    # matches at a block's first bytes: one literal, then copies of it
    d = dw.Deflate()
    d.fixed([0x41, (258, 1), (3, 2), 0x42, (17, 2), (258, 259)], final=True)
    add("lz_first_bytes", "C", [_frame(d)], lambda r: r[0][0][0].matches[0][0] == 1)
    # outputs across the wave LZ kernel's 4 KB flushes: long matches at near, middle and far distances
    d = dw.Deflate()
    d.stored(_rand(rng, 5000))
    toks, n = [], 5000
    while n < 40000:
        L, dist = rng.choice([258, 255, 131, 64]), rng.choice([1, 7, 64, 240, 241, 4096, 5000])
        toks += [rng.randrange(256), (L, dist)]
        n += L + 1
    d.dynamic(toks, final=True, header="zlib")
    add("lz_across_4k_flushes", "C", [_frame(d)],
        lambda r: sum(1 for m in r[0][0][1].matches if m[0] // 4096 != (m[0] + m[1] - 1) // 4096) >= 5)

    # each block's output starting at every phase 0..63 mod 64 (ISIZE = 1 mod 64): matches at its first and last bytes
    for j in range(64):
        isize = 961 + 64 * (j % 3)
        toks, n = [rng.randrange(256)], 1
        while n < isize - 600:
            dist = rng.choice([1, 2, 3, 5, 8, 9, 31, 63, 64, 65, 200, 240, 241, 300, 500])
            if dist <= n:
                L = rng.choice([3, 4, 7, 8, 15, 16, 17, 63, 64, 65, 258])
                toks.append((L, dist))
                n += L
            toks.append(rng.randrange(256))
            n += 1
        rest = isize - n
        toks += [rng.randrange(256) for _ in range(rest - 258)] + [(258, rng.choice([1, 3, 64, 240, 241]))]
        d = dw.Deflate()
        (d.fixed if j % 2 else d.dynamic)(toks, final=True)
        add("phase_%02d" % j, "phase", [_frame(d)], lambda r, isize=isize: r[0][1] and len(r[0][1]) == isize and r[0][0][0].matches[-1][0] + 258 == isize)

    # ---- the fast path's sequence-stream slot: the same BGZF block once just inside its slot, once one byte over
    d = dw.Deflate()
    for _ in range(292):                                       # 292 one-literal dynamic blocks (5 stream bytes each) + 3 stored bytes
        d.dynamic([rng.randrange(256)], header="plain")
    d.stored(_rand(rng, 3), final=True)
    slot_block = _frame(d)
    fillers = []
    for f in (3, 8, 1, 2, 4, 5, 6, 7):
        dd = dw.Deflate()
        dd.stored(_rand(rng, f), final=True)
        fillers.append(_frame(dd))
    members = []
    for fb in fillers:
        members += [fb, slot_block]
    add("slot_edges", "slot", members, lambda r: slot_check(r))

    # ---- D. framing
    # ISIZE 65,536 in a block of exactly 65,536 bytes; ISIZE 65,535
    for total in (65536, 65535):
        stored = _rand(rng, 65535)
        for L in range(65505, 65000, -1):                      # a stored block, then matches for the rest: 26 + 5 + L + theirs
            d = dw.Deflate()
            d.stored(stored[:L])
            n, toks = L, []
            while n < total:
                k = min(258, total - n) if total - n not in (259, 260) else 100
                toks.append((k, 1 + n % 4000) if k >= 3 else rng.randrange(256))
                n += k if k >= 3 else 1
            d.fixed(toks, final=True)
            if len(d.getvalue()) <= 65536 - 26:
                break
        add("isize_%d" % total, "D", [_frame(d)], lambda r, total=total: len(r[0][1]) == total)
    # non-EOF empty blocks with valid streams: fixed EOB only, stored LEN 0, dynamic EOB only -- between data blocks
    empties = []
    for kind in ("fixed", "stored", "dynamic"):
        d = dw.Deflate()
        {"fixed": lambda: d.fixed([]), "stored": lambda: d.stored(b""), "dynamic": lambda: d.dynamic([], header="plain")}[kind]()
        if kind == "stored":
            d.fixed([], final=True)
        else:
            d.stored(b"", final=True)
        empties.append(_frame(d))
    data_blk = dw.Deflate()
    data_blk.fixed(dw.greedy_lz77(text[:2000]), final=True)
    db = _frame(data_blk)
    add("empty_blocks", "D", [db, empties[0], db, empties[1], empties[2], db],
        lambda r: [len(x[1]) for x in r] == [2000, 0, 2000, 0, 0, 2000] and all(not x[0][0].final for x in r[1::3] + r[4:5]))
    # XLEN > 6: BC behind other subfields
    d = dw.Deflate()
    d.dynamic(dw.greedy_lz77(text[5000:9000]), final=True, header="combined")
    add("extra_subfields", "D", [_frame(d, extra=[(65, 66, b"xyz"), (1, 2, b"")]), _frame(d, extra=[(90, 90, bytes(100))])],
        lambda r: True)
    return cases


def slot_check(results):
    """Slot group: the block of 292 one-literal DEFLATE blocks fits its slot exactly and misses it by one byte, in the lane
    LZ kernel's stream form and in the SPLIT form (+ its pad) -- with the launch laid out as the group is."""
    sizes = [len(out) for _b, out in results]
    lay = slot_layout(sizes)
    lane, split = set(), set()
    for k in range(1, len(results), 2):
        z = _stream_size(results[k][0])
        cap, pad = lay[k]
        lane.add(z - cap)
        split.add(pad + z - cap)
    return {0, 1} <= lane and {0, 1} <= split


# ---------------------------------------------------------------------------------------------------------------------
# malformed blocks: one defect each, every one checked explicitly by all five decoders

def _good(rng, n=3000):
    d = dw.Deflate()
    d.dynamic(dw.greedy_lz77(_rand(rng, n, b"ACGT")), final=True)
    return _frame(d)


def malformed(seed=7):
    """-> [(name, bad BGZF block)]; each decodes to nothing valid (zlib raises, or the footer's ISIZE disagrees)."""
    rng = random.Random(seed)
    out = []

    def add(name, d, isize=None, data=None):
        out.append((name, dw.bgzf(d.getvalue(), bytes(d.data) if data is None else data, isize=isize)))

    d = dw.Deflate(); d.fixed([65, 66]); d.raw(1, 1); d.raw(3, 2); d.pad_bits(20)
    add("btype3", d, isize=2)
    d = dw.Deflate(); d.stored(b"abcd", final=True, nlen=0xFFFF ^ 5)
    add("stored_nlen", d)
    lit = _lengths(rng, 286, range(286))
    dist = _lengths(rng, 30, range(30))
    for name, kw in (("hlit287", dict(hlit=287)), ("hdist31", dict(hdist=31))):
        d = dw.Deflate()
        d.dynamic([65, 66, 67], lit_lens=lit + [0, 0], dist_lens=dist + [0, 0], final=True, **kw)
        add(name, d)
    over = list(lit); over[0] = 1; over[1] = 1           # over-subscribed literal / length code
    d = dw.Deflate(); d.dynamic([], lit_lens=over, dist_lens=dist, final=True, eob=False); d.pad_bits(64)
    add("oversubscribed_lit", d, isize=10)
    dover = list(dist); dover[0] = 1; dover[1] = 1; dover[2] = 1
    d = dw.Deflate(); d.dynamic([], lit_lens=lit, dist_lens=dover, final=True, eob=False); d.pad_bits(64)
    add("oversubscribed_dist", d, isize=10)
    d = dw.Deflate(); d.dynamic([65, 66], final=True, header="plain", cl_lens=[1] * 19, eob=False); d.pad_bits(64)
    add("oversubscribed_precode", d, isize=2)
    seq_runs = [(16, 0)] + [(8, None)] * 254 + [(0, None)]
    d = dw.Deflate(); d.dynamic([], lit_lens=[8] * 257, dist_lens=[0], runs=seq_runs, hlit=257, hdist=1, final=True, eob=False); d.pad_bits(64)
    add("sixteen_first", d, isize=10)
    runs = [(8, None)] * 256 + [(9, None), (9, None), (18, 127)]
    d = dw.Deflate(); d.dynamic([], lit_lens=[8] * 256 + [9, 9], dist_lens=[0], runs=runs, hlit=258, hdist=1, final=True, eob=False); d.pad_bits(64)
    add("repeat_past_end", d, isize=10)
    noeob = [8] * 256 + [0]
    d = dw.Deflate(); d.dynamic([], lit_lens=noeob, dist_lens=[1], final=True, header="plain", eob=False); d.pad_bits(64)
    add("eob_length0", d, isize=10)
    for s in (286, 287):
        d = dw.Deflate(); d.fixed([65, 66, ("sym", s)], final=True); d.pad_bits(16)
        add("fixed_lit%d" % s, d, isize=2)
    for s in (30, 31):
        d = dw.Deflate(); d.fixed([65, 66, ("sym", 257), ("dsym", s)], final=True); d.pad_bits(16)
        add("fixed_dist%d" % s, d, isize=5)
    d = dw.Deflate(); d.fixed([65, 66, (5, 3)], final=True)
    add("distance_too_far", d, isize=7, data=b"ABBBBBB")
    good = _good(rng, 2000)
    pd = payload(good[0])
    out.append(("isize_short", dw.bgzf(pd, good[1], isize=len(good[1]) - 1)))
    out.append(("isize_long", dw.bgzf(pd, good[1], isize=len(good[1]) + 1)))
    d = dw.Deflate(); d.fixed(dw.greedy_lz77(_rand(rng, 500, b"AC")))
    add("no_final_block", d)
    out.append(("isize0_with_bytes", dw.bgzf(pd, b"", isize=0, crc=0)))
    d = dw.Deflate(); d.raw(1, 1); d.raw(3, 2); d.pad_bits(5)
    add("isize0_garbage", d, isize=0)
    return out


def good_blocks(seed=8, n=4):
    rng = random.Random(seed)
    return [_good(rng, rng.randint(100, 5000)) for _ in range(n)]
