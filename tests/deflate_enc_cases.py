"""Inputs of the BGZF encoder (csrc/svx_deflate.hip), shared by the host model's test (tests/test_bgzf_deflate_cpu.py) and the device's
(tests/test_gpu_bgzf_deflate.py), and what every member must satisfy -- checked with zlib and struct only.

A planted repeat lies in bytes drawn uniformly from 0 .. 143: every literal then costs exactly 8 bits in the fixed code, the fixed form
of the block is never larger than the stored one, and the match saves bits -- the parse has to carry it, and :func:`tokens` finds it
in the member."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 0xFF00
PARTS = 8                             # processes the host program's file blocks are shared out to
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
# every length code's first length and the last length of the code in front of it (its extra bits all ones), 257 = code 284's last
LENGTHS = sorted(set(LEN_BASE) | {b - 1 for b in LEN_BASE[1:]})
# the same for the distance codes; 32,768 = code 29's last
DISTANCES = sorted(set(DIST_BASE) | {b - 1 for b in DIST_BASE[1:]} | {32768})
PLANT_LEN = 200                       # the repeat planted for a distance case
PLANT_DIST = 20                       # the distance of the repeat planted for a length case: source and copy in one wave of 64 positions


def _noise(rng, n):
    return rng.integers(0, 144, n, dtype=np.uint8)


def planted(length, dist, seed):
    """A block of bytes 0 .. 143 with ONE repeat: the ``length`` bytes at position ``at`` copy those ``dist`` in front of them, the bytes
    around both differ.  -> (bytes, at).  ``at`` is 40 behind a multiple of 64 for dist < 64 (source and copy in one wave), a multiple of
    64 otherwise."""
    rng = np.random.default_rng(seed)
    at = (dist + 100 + 63) // 64 * 64 + (40 if dist < 64 else 0)
    buf = _noise(rng, at + length + 100)
    if buf[at - 1] == buf[at - dist - 1]:                       # the repeat does not begin earlier
        buf[at - 1] = (int(buf[at - 1]) + 1) % 144
    for k in range(length):
        buf[at + k] = buf[at - dist + k]
    if buf[at + length] == buf[at - dist + length]:             # and ends here
        buf[at + length] = (int(buf[at + length]) + 1) % 144
    return buf.tobytes(), at


class Case:
    def __init__(self, name, data, stored=None, max_member=None, want_token=None, no_long_match=False):
        self.name, self.data, self.stored, self.max_member, self.want_token, self.no_long_match = name, bytes(data), stored, max_member, want_token, no_long_match


def crafted():
    """-> [Case].  ``stored``: what the member's block type must be (None: either), ``max_member``: a bound on its bytes,
    ``want_token``: (length or None, distance or None) of a match the member must hold, ``no_long_match``: no match of 8 bytes or more."""
    rng = np.random.default_rng(11)
    out = [Case("empty", b"", stored=False, max_member=28)]
    for n in (1, 2, 3, 4):
        out.append(Case("bytes_%d" % n, bytes(range(65, 65 + n))))
    out.append(Case("full_text", (b"ACGTTGCAAC" * 7000)[:BLOCK], stored=False))
    out.append(Case("all_values_once", bytes(range(256))))                      # 144 x 8 + 112 x 9 bits: stored is smaller
    out.append(Case("all_values_twice", bytes(range(256)) * 2, stored=False, want_token=(256, 256)))      # literals of 8 and of 9 bits in the fixed code
    out.append(Case("high_values_repeated", bytes(range(144, 256)) * 3, stored=False))
    # 1 literal + 253 matches of 258 + 1 of 5 = 3,319 bits = 415 bytes of payload (zlib, Z_FIXED: 416)
    out.append(Case("equal_0xFF00", b"\x07" * BLOCK, stored=False, max_member=512, want_token=(258, 1)))
    for r in (0, 1, 2, 3):
        out.append(Case("run_tail_%d" % r, b"k" * (1 + 2 * 258 + r), stored=False, want_token=(258, 1)))
    far, _at = planted(PLANT_LEN, 32768, 21)
    out.append(Case("only_source_at_32768", far, stored=False, want_token=(None, 32768)))
    over, _at = planted(PLANT_LEN, 32769, 22)
    out.append(Case("only_source_at_32769", over, no_long_match=True))
    for length in LENGTHS:
        data, _at = planted(length, PLANT_DIST, 100 + length)
        out.append(Case("length_%d" % length, data, stored=False, want_token=(length, PLANT_DIST)))
    for dist in DISTANCES:
        data, _at = planted(PLANT_LEN, dist, 1000 + dist)
        out.append(Case("distance_%d" % dist, data, stored=False, want_token=(None, dist)))
    out.append(Case("random_0xFF00", rng.integers(0, 256, BLOCK, dtype=np.uint8).tobytes(), stored=True, max_member=65311))
    out.append(Case("random_1000", rng.integers(0, 256, 1000, dtype=np.uint8).tobytes(), stored=True, max_member=1031))
    return out


def file_blocks(stream):
    """The 0xFF00-byte blocks of an inflated BAM stream."""
    return [stream[at:at + BLOCK] for at in range(0, len(stream), BLOCK)]


def layout(blocks, lead=1):
    """The blocks end to end behind ``lead`` bytes (the first block starts at an odd offset) -> (stream bytes, uint64 offsets [n + 1])."""
    off = np.zeros(len(blocks) + 1, np.uint64)
    off[0] = lead
    off[1:] = lead + np.cumsum([len(b) for b in blocks], dtype=np.uint64)
    return b"\xee" * lead + b"".join(blocks), off


def tokens(payload):
    """The tokens of ONE final fixed-Huffman DEFLATE block -> [(length, distance)] of its matches and the number of literals; an own
    bit-by-bit decoder (codes most significant bit first, extra bits least significant bit first)."""
    bits = np.unpackbits(np.frombuffer(payload, np.uint8), bitorder="little").tolist()
    p = 3
    assert list(bits[:3]) == [1, 1, 0]

    def code(n):
        nonlocal p
        v = 0
        for b in bits[p:p + n]:
            v = v << 1 | int(b)
        p += n
        return v

    def extra(n):
        nonlocal p
        v = 0
        for i, b in enumerate(bits[p:p + n]):
            v |= int(b) << i
        p += n
        return v

    matches, literals = [], 0
    while True:
        v = code(7)
        if v <= 0x17:
            sym = 256 + v
        else:
            v = v << 1 | code(1)
            if 0x30 <= v <= 0xBF:
                sym = v - 0x30
            elif 0xC0 <= v <= 0xC7:
                sym = 280 + v - 0xC0
            else:
                v = v << 1 | code(1)
                assert 0x190 <= v <= 0x1FF
                sym = 144 + v - 0x190
        if sym == 256:
            break
        if sym < 256:
            literals += 1
            continue
        assert sym <= 285
        length = LEN_BASE[sym - 257] + extra(LEN_EXTRA[sym - 257])
        d = code(5)
        assert d < 30
        matches.append((length, DIST_BASE[d] + extra(DIST_EXTRA[d])))
    assert len(payload) == (p + 7) // 8
    return matches, literals


def check_member(member, data, case=None):
    """Everything a member owes its input.  -> True where its block is stored."""
    name = case.name if case is not None else "block"
    assert member[:16] == HEADER, name
    assert struct.unpack_from("<H", member, 16)[0] + 1 == len(member) <= 65536, name
    payload = member[18:-8]
    assert zlib.decompress(payload, -15) == data, name
    d = zlib.decompressobj(-15)
    d.decompress(payload)
    assert d.eof and d.unused_data == b"", name
    assert struct.unpack_from("<II", member, len(member) - 8) == (zlib.crc32(data) & 0xFFFFFFFF, len(data)), name
    assert len(member) <= len(data) + 31, name                   # never larger than the stored form
    kind = payload[0] & 7
    assert kind in (1, 3), name                                   # one FINAL block, stored or fixed
    is_stored = kind == 1
    if is_stored:
        assert len(member) == len(data) + 31, name
    if case is not None:
        if case.stored is not None:
            assert is_stored == case.stored, name
        if case.max_member is not None:
            assert len(member) <= case.max_member, (name, len(member))
        if case.want_token is not None or case.no_long_match:
            matches, _lit = ([], 0) if is_stored else tokens(payload)
            assert all(3 <= l <= 258 and 1 <= dd <= 32768 for l, dd in matches), name
            if case.want_token is not None:
                wl, wd = case.want_token
                assert any((wl is None or l == wl) and (wd is None or dd == wd) for l, dd in matches), (name, case.want_token)
            if case.no_long_match:
                assert not any(l >= 8 for l, _dd in matches), name
    return is_stored


# ---- the files' blocks and the host program (tools/hostwave/deflate_main.cpp)
def bam_blocks(tmp_dir):
    """-> [(name, block bytes)]: the inflated streams of the golden BAMs and of three index-build files, cut every 0xFF00 bytes."""
    from tests import baicases, helpers, htslike
    out = []
    streams = [(n, baicases.walk(os.path.join(helpers.GOLDEN, n + ".bam")).stream) for n in ("collect_small", "ont_small")]
    path = str(tmp_dir / "straddling.bam")
    htslike.write_bam(path, baicases.REFS, baicases.short_records(seed=4), level=1, policy="stream", index=False)
    streams.append(("straddling", baicases.walk(path).stream))
    streams.append(("long", baicases.write_long(str(tmp_dir / "long.bam"))[0].stream))
    streams.append(("decoy", baicases.write_decoy(str(tmp_dir / "decoy.bam"))[0].stream))
    for name, s in streams:
        out += [("%s[%d]" % (name, i), b) for i, b in enumerate(file_blocks(s))]
    return out


def write_cases(path, blocks):
    stream, off = layout(blocks)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blocks)) + off.tobytes() + stream)


def read_members(path):
    raw = open(path, "rb").read()
    n = struct.unpack_from("<I", raw)[0]
    lens = np.frombuffer(raw, np.uint32, n, 4).tolist()
    stored = np.frombuffer(raw, np.uint32, n, 4 + 4 * n).tolist()
    body, at, out = raw[4 + 8 * n:], 0, []
    for k in lens:
        out.append(body[at:at + k])
        at += k
    assert at == len(body)
    return out, stored


def build_host(tmp_dir, sanitize=False):
    """The host program, stand-alone -> its path.  ``sanitize``: under AddressSanitizer and UBSan (the CPU test); plain -O2 is all a
    comparison of bytes needs (the GPU test)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_dir / "deflate_host")
    checks = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O2"] + checks + ["-o", out, os.path.join(ROOT, "tools", "hostwave", "deflate_main.cpp"), "-lz"])
    return out


def run_host(program, tmp_dir, cases, files, case_orders, file_orders):
    """The host program on the crafted cases in ``case_orders`` thread orders and on the files' blocks in ``file_orders``, the latter
    shared out to PARTS processes that run side by side -> per order (members, stored flags), crafted cases first, then the files'
    blocks where that order ran on them."""
    d = tmp_dir
    jobs = [("cases", [c.data for c in cases], case_orders)] + [("files%d" % k, [b for _n, b in files[k::PARTS]], file_orders) for k in range(PARTS)]
    procs = []
    for name, blocks, orders in jobs:
        write_cases(str(d / (name + ".bin")), blocks)
        procs.append(subprocess.Popen([program, str(d / (name + ".bin")), str(d / name), str(orders)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for p in procs:
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0 and "FAILED" not in out and "deflate_host: ok" in out, out[-3000:] + err[-3000:]
    per_order = []
    for o in range(case_orders):
        got, stored = read_members(str(d / ("cases.%d" % o)))
        if o < file_orders:
            got_f, stored_f = [None] * len(files), [None] * len(files)
            for k in range(PARTS):
                got_f[k::PARTS], stored_f[k::PARTS] = read_members(str(d / ("files%d.%d" % (k, o))))
            got, stored = got + got_f, stored + stored_f
        per_order.append((got, stored))
    return per_order
