"""The DEFLATE writer of the tests (tests/deflate_writer.py) and the catalogue built with it (tests/inflate_cases.py), on the
CPU: every stream decodes with zlib to exactly the bytes its case intends, the host BGZF reader agrees on the framed blocks,
and every case really holds the construct it is there for -- parsed back out of its own bytes, so that an edit cannot turn
a case into an ordinary stream without this file noticing.  The malformed blocks are rejected by zlib."""
import random
import zlib

import pytest

from svision_amd.io import bam
from tests import deflate_writer as dw
from tests import inflate_cases as ic


@pytest.fixture(scope="module")
def cases():
    return ic.build()


def test_catalogue_size_and_names(cases):
    names = [c.name for c in cases]
    assert len(names) == len(set(names))
    assert {c.group for c in cases} == {"A", "B", "C", "D", "phase", "slot"}
    assert 120 <= sum(len(c.members) for c in cases) <= 260


def test_every_case_decodes_to_its_bytes_and_holds_its_feature(cases):
    for c in cases:
        parsed = []
        for block, data in c.members:
            cdata = ic.payload(block)
            assert zlib.decompress(cdata, -15) == data, c.name
            assert bam.bgzf_decompress(block) == data, c.name
            blocks, out = dw.inspect(cdata)
            assert out == data, c.name
            parsed.append((blocks, out))
        assert c.feature(parsed), c.name


def test_framing(cases):
    by = {c.name: c for c in cases}
    assert max(len(b) for b, _d in by["isize_65536"].members) == 65536                  # BSIZE at its maximum
    assert len(by["isize_65535"].members[0][1]) == 65535
    for block, _d in by["extra_subfields"].members:
        xlen = block[10] | block[11] << 8
        assert xlen > 6 and block[12:14] != b"BC"
    raw = b"".join(b for c in cases for b, _d in c.members)
    assert bam.bgzf_decompress(raw + bam._BGZF_EOF) == b"".join(d for c in cases for _b, d in c.members)


def test_slot_layout_matches_the_kernel_formula():
    lay = ic.slot_layout([3, 295])
    assert lay[0] == (3 + 1 + 1024, 0)
    assert lay[1] == (298 + 149 - 4 + 1024, (-(256 + 3 + 1 + 1024)) & 3)


def test_writer_modes_round_trip():
    rng = random.Random(3)
    data = bytes(rng.choice(b"ACGTTTTTTTTTTTTTTTTTTTTTTTTTT") for _ in range(30000))
    toks = dw.greedy_lz77(data)
    assert dw.apply_tokens(toks) == data
    for mode in ("zlib", "combined", "plain", "max-runs"):
        for hclen in ("min", "full"):
            for hlit, hdist in ((None, None), (286, 30)):
                d = dw.Deflate()
                d.fixed(toks[:50])
                d.stored(b"")
                d.dynamic(toks[50:], header=mode, hclen=hclen, hlit=hlit, hdist=hdist)
                d.stored(b"\x00" * 65535, final=True)
                s = d.getvalue()
                assert zlib.decompress(s, -15) == data + b"\x00" * 65535 == bytes(d.data)
                blocks, _out = dw.inspect(s)
                b = blocks[2]
                assert b.hclen == 19 if hclen == "full" else b.hclen < 19
                if mode == "plain":
                    assert all(s < 16 for s, _x, _at in b.runs)
                if mode == "zlib":
                    assert not dw.crossing_runs(b)
                if hlit:
                    assert (b.hlit, b.hdist) == (286, 30)


def test_length_limit_keeps_codes_complete():
    fib = [1, 1]
    while len(fib) < 286:
        fib.append(fib[-1] + fib[-2])
    for n in (20, 30, 286):
        lens = dw.huffman_lengths(fib[:n])
        assert max(lens) == 15 and dw.kraft(lens) == 1 << 15
    assert dw.huffman_lengths([0, 5, 0]) == [0, 1, 0]                          # one symbol: an incomplete code of length 1
    assert dw.kraft(dw.huffman_lengths([0, 5, 0], limit=7, complete=True), 7) == 1 << 7


def test_the_bit_writer_is_fast_enough():
    import time
    rng = random.Random(4)
    data = bytes(rng.getrandbits(8) for _ in range(1 << 20))
    t = time.time()
    for _ in range(5):
        d = dw.Deflate()
        d.fixed(list(data), final=True)
        assert len(d.getvalue()) > len(data)
    assert time.time() - t < 30


def test_malformed_blocks_are_invalid():
    for name, block in ic.malformed():
        cdata = ic.payload(block)
        isize = int.from_bytes(block[-4:], "little")
        try:
            out = zlib.decompress(cdata, -15)
        except zlib.error:
            continue
        assert len(out) != isize, name                                         # decodes, but not to what its footer says


def test_adversarial_encoder_holds_its_constructs():
    rng = random.Random(9)
    data = bytes(rng.choice(b"ACGT") for _ in range(20000)) + bytes(rng.getrandbits(8) for _ in range(3000)) + b"N" * 20000
    cdata = dw.adversarial(data)
    assert zlib.decompress(cdata, -15) == data
    blocks, out = dw.inspect(cdata)
    assert out == data
    dyn = [b for b in blocks if b.btype == 2]
    assert {b.btype for b in blocks} == {0, 1, 2}
    assert any(dw.crossing_runs(b) for b in dyn)
    assert any(sum(1 for l in b.dist_lens if l) == 1 and b.matches for b in dyn)
    assert {len(b.matches) + (b.out1 - b.out0) - sum(m[1] for m in b.matches) for b in dyn[:2]} == {1, 7}       # tokens per block
