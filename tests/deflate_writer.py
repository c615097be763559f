"""An RFC 1951 DEFLATE writer (and a reader of its own output) for the tests: every legal construct an encoder MAY emit,
not only what zlib or libdeflate happen to -- code-length runs that cross from the literal / length lengths into the
distance lengths (3.2.7 treats the two arrays as one sequence), single and absent distance codes, end-of-block-only dynamic
blocks, any HLIT / HDIST / HCLEN, 15-bit codes, stored blocks at every bit phase, explicit (length, distance) tokens -- and
BGZF framing with any ISIZE and extra gzip subfields in front of BC.

Shares no code with svision_amd: ``struct``, ``zlib`` (CRC32 only) and ``heapq``.  ``inspect`` parses a stream back into
what it holds (block headers, runs of the code-length code, bit positions, tokens), so that a test can assert that the
feature a case claims is really in its bytes.

Tokens: an int 0..255 is a literal, a tuple (length, distance) a match; ("sym", s) / ("dsym", s) emit a raw literal /
length or distance symbol (malformed streams only)."""
import heapq
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8

_LEN_CODE = [0] * 259                      # length -> index into LEN_BASE
for _i in range(29):
    for _l in range(LEN_BASE[_i], (LEN_BASE[_i + 1] if _i < 28 else 259)):
        _LEN_CODE[_l] = _i
_LEN_CODE[258] = 28                        # (258 is code 285, never 284 + 31)


def dist_code(d):
    lo, hi = 0, 29
    while lo < hi:                         # the last base <= d
        mid = (lo + hi + 1) // 2
        if DIST_BASE[mid] <= d:
            lo = mid
        else:
            hi = mid - 1
    return lo


def canonical(lens):
    """Code lengths -> canonical codes (RFC 1951 3.2.2), MSB-first integers; 0 where the length is 0."""
    count = [0] * 16
    for l in lens:
        if l:
            count[l] += 1
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1 if l > 1 else 0
        nxt[l] = code
    out = []
    for l in lens:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(0)
    return out


def kraft(lens, limit=15):
    """Sum of 2^(limit - l) over the used lengths: 2^limit = complete, more = over-subscribed."""
    return sum(1 << (limit - l) for l in lens if l)


def huffman_lengths(freqs, limit=15, complete=False):
    """Frequencies -> code lengths of at most ``limit`` bits (Huffman, then the usual depth-limiting heuristic).  One used
    symbol: length 1 (an incomplete code, legal for a single literal / length or distance code); ``complete`` then adds a
    second symbol of length 1, which a code-length code needs."""
    used = [i for i, f in enumerate(freqs) if f]
    lens = [0] * len(freqs)
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0]] = 1
        if complete:
            lens[1 if used[0] == 0 else 0] = 1
        return lens
    heap = [(freqs[i], i, (i,)) for i in used]
    heapq.heapify(heap)
    tie = len(freqs)
    while len(heap) > 1:
        fa, _ta, a = heapq.heappop(heap)
        fb, _tb, b = heapq.heappop(heap)
        for s in a + b:
            lens[s] += 1
        heapq.heappush(heap, (fa + fb, tie, a + b))
        tie += 1
    if max(lens) > limit:
        lens = [min(l, limit) for l in lens]
        full = 1 << limit
        while kraft(lens, limit) > full:    # lengthen the deepest code still below the limit
            s = max((s for s in used if lens[s] < limit), key=lambda s: (lens[s], freqs[s] * -1))
            lens[s] += 1
        while kraft(lens, limit) < full:    # fill what is left by shortening the longest codes that may
            k = kraft(lens, limit)
            s = max((s for s in used if lens[s] > 1 and k + (1 << (limit - lens[s])) <= full), key=lambda s: (lens[s], -freqs[s]))
            lens[s] -= 1
    return lens


class BitWriter:
    """LSB-first bits into bytes; a small int accumulator that is flushed as whole bytes."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def pos(self):
        return 8 * len(self.out) + self.n

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 2048:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def code(self, code, length):
        """A Huffman code: its bits go out MSB first."""
        self.bits(int(format(code, "0%db" % length)[::-1], 2), length)

    def align(self):
        if self.n & 7:
            self.bits(0, 8 - (self.n & 7))

    def getvalue(self):
        k = (self.n + 7) >> 3
        return bytes(self.out) + (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")


def apply_tokens(tokens, history=b""):
    """What a token list decodes to behind ``history`` (bytes)."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t
            assert 1 <= dist <= len(out), (t, len(out))
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out[len(history):])


def greedy_lz77(data, history=b"", window=32768, min_match=3, max_match=258):
    """A plain greedy LZ77 (one candidate per 3-byte hash): literals and (length, distance) tokens."""
    buf = bytes(history) + bytes(data)
    last = {}
    for i in range(max(0, len(history) - window), len(history) - 2):
        last[buf[i:i + 3]] = i
    out, i, n = [], len(history), len(buf)
    while i < n:
        key = buf[i:i + 3]
        j = last.get(key) if len(key) == 3 else None
        best = 0
        if j is not None and i - j <= window:
            lim = min(max_match, n - i)
            while best + 16 <= lim and buf[j + best:j + best + 16] == buf[i + best:i + best + 16]:
                best += 16
            while best < lim and buf[j + best] == buf[i + best]:
                best += 1
        if best >= min_match:
            out.append((best, i - j))
            for k in range(i, min(i + best, n - 2)):
                last[buf[k:k + 3]] = k
            i += best
        else:
            if len(key) == 3:
                last[key] = i
            out.append(buf[i])
            i += 1
    return out


def token_symbols(tokens):
    """-> literal / length symbol frequencies [286], distance symbol frequencies [30] (EOB counted once)."""
    lf, df = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        elif t[0] == "sym":
            pass
        elif t[0] == "dsym":
            pass
        else:
            lf[257 + _LEN_CODE[t[0]]] += 1
            df[dist_code(t[1])] += 1
    lf[256] += 1
    return lf, df


def rle_lengths(seq, mode, split=None):
    """A code-length sequence -> [(symbol, extra value)] of the code-length code.
    ``zlib``: the two arrays run-length coded separately (``split`` = HLIT); ``combined``: runs cross the boundary;
    ``plain``: no 16 / 17 / 18; ``max-runs``: 18 x 138 where it can, 17 x 3, 16 x 6 and 16 repeating a zero."""
    if mode == "plain":
        return [(v, None) for v in seq]
    if mode == "zlib":
        return rle_lengths(seq[:split], "combined") + rle_lengths(seq[split:], "combined")
    out, i, n, prev = [], 0, len(seq), None
    while i < n:
        v = seq[i]
        r = 1
        while i + r < n and seq[i + r] == v:
            r += 1
        if mode == "max-runs":
            if v == 0 and r >= 11:
                k = min(r, 138)
                out.append((18, k - 11))
            elif prev == v and r >= 3:
                k = min(r, 6)
                out.append((16, k - 3))
            elif v == 0 and r >= 3:
                k = 3
                out.append((17, 0))
            else:
                k = 1
                out.append((v, None))
            prev = v
            i += k
            continue
        if v == 0 and r >= 3:
            k = min(r, 138)
            out.append((18, k - 11) if k >= 11 else (17, k - 3))
            i += k
        else:
            out.append((v, None))
            i += 1
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k - 3))
                i += k
                r -= k
        prev = v
    return out


_CL_EXTRA = {16: 2, 17: 3, 18: 7}


class Deflate:
    """A raw DEFLATE stream, block after block."""

    def __init__(self):
        self.w = BitWriter()
        self.data = bytearray()            # what the stream decodes to so far

    def raw(self, value, n):
        self.w.bits(value, n)

    def pad_bits(self, n):
        self.w.bits(0, n)

    def stored(self, data, final=False, nlen=None):
        assert len(data) <= 65535
        self.w.bits(int(final), 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
        for b in bytes(data):
            self.w.bits(b, 8)
        self.data += data

    def _tokens(self, tokens, lcode, llen, dcode, dlen, eob=True):
        w = self.w
        out = self.data
        for t in tokens:
            if isinstance(t, int):
                w.code(lcode[t], llen[t])
                out.append(t)
            elif t[0] == "sym":
                w.code(lcode[t[1]], llen[t[1]])
            elif t[0] == "dsym":
                w.code(dcode[t[1]], dlen[t[1]])
            else:
                length, dist = t
                li = _LEN_CODE[length]
                w.code(lcode[257 + li], llen[257 + li])
                if LEN_EXTRA[li]:
                    w.bits(length - LEN_BASE[li], LEN_EXTRA[li])
                di = dist_code(dist)
                w.code(dcode[di], dlen[di])
                if DIST_EXTRA[di]:
                    w.bits(dist - DIST_BASE[di], DIST_EXTRA[di])
                if dist <= len(out):
                    for _ in range(length):
                        out.append(out[-dist])
        if eob:
            w.code(lcode[256], llen[256])

    def fixed(self, tokens, final=False, eob=True):
        self.w.bits(int(final), 1)
        self.w.bits(1, 2)
        self._tokens(tokens, canonical(FIXED_LIT), FIXED_LIT, canonical([5] * 32), [5] * 32, eob)

    def dynamic(self, tokens, final=False, lit_lens=None, dist_lens=None, header="zlib", hclen="min", hlit=None, hdist=None,
                runs=None, cl_lens=None, eob=True):
        """``lit_lens`` / ``dist_lens``: the code lengths verbatim (else from the tokens' frequencies, at most 15 bits);
        ``hlit`` / ``hdist``: how many lengths are sent (default: up to the last used symbol); ``runs``: the code-length
        code's symbols verbatim [(symbol, extra value)]; ``cl_lens``: the code-length code's 19 lengths verbatim."""
        lf, df = token_symbols(tokens)
        if lit_lens is None:
            lit_lens = huffman_lengths(lf)
        if dist_lens is None:
            dist_lens = huffman_lengths(df)
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        nl = hlit if hlit is not None else max(257, max(i for i, l in enumerate(lit_lens) if l) + 1)
        used_d = [i for i, l in enumerate(dist_lens) if l]
        nd = hdist if hdist is not None else max(1, used_d[-1] + 1 if used_d else 1)
        lit_lens += [0] * (max(nl, 288) - len(lit_lens))
        dist_lens += [0] * (max(nd, 32) - len(dist_lens))
        seq = lit_lens[:nl] + dist_lens[:nd]
        if runs is None:
            runs = rle_lengths(seq, header, nl)
        if cl_lens is None:
            cf = [0] * 19
            for s, _x in runs:
                cf[s] += 1
            cl_lens = huffman_lengths(cf, limit=7, complete=True)
        ncl = 19 if hclen == "full" else max(4, max(k for k in range(19) if cl_lens[CLEN_ORDER[k]]) + 1)
        w = self.w
        w.bits(int(final), 1)
        w.bits(2, 2)
        w.bits(nl - 257, 5)
        w.bits(nd - 1, 5)
        w.bits(ncl - 4, 4)
        for k in range(ncl):
            w.bits(cl_lens[CLEN_ORDER[k]], 3)
        ccode = canonical(cl_lens)
        for s, x in runs:
            w.code(ccode[s], cl_lens[s])
            if s >= 16:
                w.bits(x, _CL_EXTRA[s])
        self._tokens(tokens, canonical(lit_lens), lit_lens, canonical(dist_lens), dist_lens, eob)

    def getvalue(self):
        return self.w.getvalue()


# ---------------------------------------------------------------------------------------------------------------------
# BGZF framing

def bgzf(cdata, data, isize=None, extra=(), crc=None):
    """One BGZF block around raw DEFLATE bytes: ``extra`` = [(si1, si2, payload bytes)] gzip subfields IN FRONT of BC;
    ``isize`` / ``crc``: the footer's fields (default: of ``data``)."""
    sub = b"".join(bytes([a, b]) + struct.pack("<H", len(p)) + bytes(p) for a, b, p in extra)
    xlen = len(sub) + 6
    total = 12 + xlen + len(cdata) + 8
    assert total <= 65536 and len(data) <= 65536, (total, len(data))      # SAMv1 4.1: a block holds at most 64 KB either way
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", xlen) + sub + b"BC\x02\x00" + struct.pack("<H", total - 1)
    return head + bytes(cdata) + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF if crc is None else crc,
                                             len(data) if isize is None else isize)


# ---------------------------------------------------------------------------------------------------------------------
# the reader: what a stream holds, for the tests' assertions

class _Bits:
    def __init__(self, data):
        self.d = bytes(data) + b"\x00" * 8
        self.limit = 8 * len(data)
        self.p = 0

    def peek(self, n):
        q = self.p >> 3
        return (int.from_bytes(self.d[q:q + 4], "little") >> (self.p & 7)) & ((1 << n) - 1)

    def get(self, n):
        if n == 0:
            return 0
        v = self.peek(n)
        self.p += n
        if self.p > self.limit:
            raise ValueError("stream ends early")
        return v


def _decoder(lens):
    codes = canonical(lens)
    table = {}
    for s, (l, c) in enumerate(zip(lens, codes)):
        if l:
            table[(l, c)] = s
    return table, max(lens) if any(lens) else 0


def _decode(br, dec):
    table, maxl = dec
    code = 0
    for l in range(1, maxl + 1):
        code = code << 1 | br.get(1)
        s = table.get((l, code))
        if s is not None:
            return s
    raise ValueError("not a code")


class Block:
    """One DEFLATE block as ``inspect`` found it.  Bit positions from the stream's first bit: ``start`` (the header),
    ``body`` (the first bit behind the header: stored data / the first token), ``end`` (behind the EOB code / the stored
    bytes); ``out0`` / ``out1`` its output range; ``runs`` [(symbol, extra, index of the first length it sets)]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def inspect(stream, history=b""):
    """Parse a raw DEFLATE stream -> ([Block], decoded bytes).  Raises ValueError on anything invalid."""
    br = _Bits(stream)
    out = bytearray(history)
    blocks = []
    while True:
        start = br.p
        final = br.get(1)
        btype = br.get(2)
        b = Block(start=start, final=final, btype=btype, out0=len(out) - len(history), matches=[], runs=[], lit_lens=None,
                  dist_lens=None, cl_lens=None, hlit=None, hdist=None, hclen=None, lit_syms=set(), dist_syms=set())
        if btype == 0:
            br.p = (br.p + 7) & ~7
            ln, nln = br.get(16), br.get(16)
            if ln ^ nln != 0xFFFF:
                raise ValueError("LEN / NLEN")
            b.body = br.p
            b.len = ln
            for _ in range(ln):
                out.append(br.get(8))
        elif btype == 3:
            raise ValueError("BTYPE 3")
        else:
            if btype == 1:
                lit_lens, dist_lens = FIXED_LIT, [5] * 32
            else:
                b.hlit, b.hdist, b.hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                cl = [0] * 19
                for k in range(b.hclen):
                    cl[CLEN_ORDER[k]] = br.get(3)
                if kraft(cl, 7) > 128:
                    raise ValueError("code-length code over-subscribed")
                if kraft(cl, 7) < 128:
                    raise ValueError("code-length code incomplete")
                b.cl_lens = cl
                cdec = _decoder(cl)
                seq = []
                n = b.hlit + b.hdist
                while len(seq) < n:
                    s = _decode(br, cdec)
                    at = len(seq)
                    if s < 16:
                        seq.append(s)
                        b.runs.append((s, None, at))
                        continue
                    x = br.get(_CL_EXTRA[s])
                    if s == 16:
                        if not seq:
                            raise ValueError("16 first")
                        v, r = seq[-1], 3 + x
                    else:
                        v, r = 0, (3 if s == 17 else 11) + x
                    if len(seq) + r > n:
                        raise ValueError("repeat past HLIT + HDIST")
                    seq += [v] * r
                    b.runs.append((s, x, at))
                lit_lens, dist_lens = seq[:b.hlit], seq[b.hlit:]
                if lit_lens[256] == 0:
                    raise ValueError("no EOB code")
                for lens in (lit_lens, dist_lens):
                    k = kraft(lens)
                    if k > 1 << 15 or (k < 1 << 15 and sum(1 for l in lens if l) > 1):
                        raise ValueError("bad code")
            b.lit_lens, b.dist_lens = list(lit_lens), list(dist_lens)
            b.body = br.p
            ldec, ddec = _decoder(lit_lens), _decoder(dist_lens)
            while True:
                s = _decode(br, ldec)
                b.lit_syms.add(s)
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                li = s - 257
                if li >= 29:
                    raise ValueError("length code %d" % s)
                length = LEN_BASE[li] + br.get(LEN_EXTRA[li])
                ds = _decode(br, ddec)
                if ds >= 30:
                    raise ValueError("distance code %d" % ds)
                b.dist_syms.add(ds)
                dist = DIST_BASE[ds] + br.get(DIST_EXTRA[ds])
                if dist > len(out):
                    raise ValueError("distance too far back")
                b.matches.append((len(out) - len(history), length, dist))
                for _ in range(length):
                    out.append(out[-dist])
        b.end = br.p
        b.out1 = len(out) - len(history)
        blocks.append(b)
        if final:
            break
        if br.p >= br.limit:
            raise ValueError("no final block")
    return blocks, bytes(out[len(history):])


def crossing_runs(b):
    """The code-length runs of a dynamic block that set lengths on both sides of HLIT: [(symbol, first index, count)]."""
    out = []
    for s, x, at in b.runs:
        if s >= 16:
            r = 3 + x if s in (16, 17) else 11 + x
            if at < b.hlit < at + r:
                out.append((s, at, r))
    return out


def adversarial(data, seed=0):
    """Raw DEFLATE of ``data`` as an encoder zlib is not: the greedy tokens cut into blocks at odd token counts, and the blocks
    in turn dynamic with combined code-length runs, stored, dynamic with max-runs and HCLEN 19, dynamic with a single distance
    code (matches at other distance codes spelt out as literals); an end-of-block-only fixed block ends the stream."""
    toks = greedy_lz77(data)
    cuts = [1, 3, 7, 31, 501, 1999, 5, 777]
    d = Deflate()
    pos, i, k = 0, 0, seed
    while i < len(toks):
        part = toks[i:i + cuts[k % len(cuts)]]
        i += len(part)
        n = sum(1 if isinstance(t, int) else t[0] for t in part)
        kind = k % 4
        k += 1
        if kind == 0:
            d.dynamic(part, header="combined", hlit=286, hdist=30)      # (all lengths sent: zero runs cross HLIT)
        elif kind == 1:
            d.stored(data[pos:pos + n])
        elif kind == 2:
            d.dynamic(part, header="max-runs", hclen="full")
        else:
            codes = [dist_code(t[1]) for t in part if not isinstance(t, int)]
            keep = max(set(codes), key=codes.count) if codes else None
            single, at = [], pos
            for t in part:
                if isinstance(t, int) or dist_code(t[1]) == keep:
                    single.append(t)
                else:
                    single += list(data[at:at + t[0]])
                at += 1 if isinstance(t, int) else t[0]
            d.dynamic(single, header="zlib")
        pos += n
    d.fixed([], final=True)
    assert bytes(d.data) == bytes(data)
    return d.getvalue()
