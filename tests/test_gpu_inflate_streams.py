"""Every device inflater (lds, private, wave, fast-lane, fast-wave and the default entry point, with its hand-over to the
wave kernel) on DEFLATE streams zlib never writes (tests/inflate_cases.py: crossing code-length runs, single / absent
distance codes, 15-bit codes, EOB at lane-segment and chunk edges, every match distance and length class at every output
phase, sequence streams at the edge of their slot, empty non-EOF blocks, extra gzip subfields), on blocks of real encoders
at other settings (libdeflate levels 1-12, zlib with small windows, memLevel 1 / 9, level and strategy switched inside a
block, flushes inside a block), and on malformed blocks -- each one flagged, its neighbours decoded exactly."""
import ctypes
import ctypes.util
import os
import zlib

import numpy as np
import pytest
import torch

from svision_amd import kernels
from svision_amd.io import bam
from tests import deflate_writer as dw
from tests import helpers
from tests import inflate_cases as ic

pytestmark = pytest.mark.gpu

VARIANTS = ["lds", "private", "wave", "fast-lane", "fast-wave", None]


def _inflate(blocks, variant, crc):
    raw = np.frombuffer(b"".join(blocks), np.uint8)
    src_off, src_len, isize, _blk = kernels.bgzf_block_table(raw)
    assert len(src_off) == len(blocks)
    padded = np.zeros((raw.size + 31) // 16 * 16, np.uint8)
    padded[:raw.size] = raw
    out, status = kernels.bgzf_inflate(torch.from_numpy(padded).cuda(), src_off, src_len, isize, wave=variant, crc=crc)
    return out.cpu().numpy().tobytes(), status.cpu().numpy(), isize


@pytest.fixture(scope="module")
def catalogue():
    groups = {}
    for c in ic.build():
        groups.setdefault(c.group, []).extend(c.members)
    return groups


@pytest.mark.parametrize("crc", [True, False])
@pytest.mark.parametrize("variant", VARIANTS)
def test_catalogue_decodes_exactly(catalogue, variant, crc):
    for group, members in catalogue.items():                    # a launch per group: "phase" and "slot" depend on the layout
        got, status, _isize = _inflate([b for b, _d in members], variant, crc)
        assert not status.any(), (group, status.tolist())
        want = b"".join(d for _b, d in members)
        if got != want:
            at = next(i for i in range(min(len(got), len(want))) if got[i] != want[i]) if len(got) == len(want) else -1
            pytest.fail("group %s: output differs (first at byte %d)" % (group, at))


# ---- real encoders at other settings, on BAM-like payloads

def _bam_payloads(tmp_path):
    from svision_amd import synth
    table, _g, _ = synth.simulate(synth.SimConfig(contigs=[("c1", 400_000)], coverage=20, seed=4), with_genome=False)
    seg = bam.encode_reference_segment(table, seq="random", seed=1)
    p = str(tmp_path / "hifi.bam")
    bam.write_bam_segments(p, table.references, table.lengths, [seg])
    raws = [bam.bgzf_decompress(open(p, "rb").read())]
    for n in ("collect_small.bam", "ont_small.bam", "hash_collect.bam"):
        raws.append(bam.bgzf_decompress(open(os.path.join(helpers.GOLDEN, n), "rb").read()))
    chunks = []
    for r in raws:
        chunks += [r[i:i + 0xFF00] for i in range(0, min(len(r), 6 * 0xFF00), 0xFF00)]
    return chunks


def _libdeflate():
    try:
        ld = ctypes.CDLL("libdeflate.so.0")
    except OSError:
        return None
    ld.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    ld.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    ld.libdeflate_deflate_compress.restype = ctypes.c_size_t
    ld.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    ld.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    return ld


def libdeflate_compress(ld, level, data):
    c = ld.libdeflate_alloc_compressor(level)
    buf = ctypes.create_string_buffer(len(data) + 1024)
    try:
        k = ld.libdeflate_deflate_compress(c, data, len(data), buf, len(buf))
        assert k
        return buf.raw[:k]
    finally:
        ld.libdeflate_free_compressor(c)


class _ZStream(ctypes.Structure):
    _fields_ = [("next_in", ctypes.c_void_p), ("avail_in", ctypes.c_uint), ("total_in", ctypes.c_ulong),
                ("next_out", ctypes.c_void_p), ("avail_out", ctypes.c_uint), ("total_out", ctypes.c_ulong),
                ("msg", ctypes.c_char_p), ("state", ctypes.c_void_p), ("zalloc", ctypes.c_void_p), ("zfree", ctypes.c_void_p),
                ("opaque", ctypes.c_void_p), ("data_type", ctypes.c_int), ("adler", ctypes.c_ulong), ("reserved", ctypes.c_ulong)]


def zlib_switching(data, params, memlevel=8, wbits=-15):
    """zlib's deflate with deflateParams called between pieces of ONE block's data: params = [(level, strategy)], one per
    equal piece (through ctypes: Python's zlib module has no deflateParams)."""
    z = ctypes.CDLL(ctypes.util.find_library("z") or "libz.so.1")
    z.zlibVersion.restype = ctypes.c_char_p
    s = _ZStream()
    assert z.deflateInit2_(ctypes.byref(s), params[0][0], 8, wbits, memlevel, params[0][1], z.zlibVersion(), ctypes.sizeof(_ZStream)) == 0
    src = ctypes.create_string_buffer(bytes(data), len(data))
    out = ctypes.create_string_buffer(2 * len(data) + 4096)
    s.next_out, s.avail_out = ctypes.addressof(out), len(out)
    step = (len(data) + len(params) - 1) // len(params)
    try:
        for k, (level, strategy) in enumerate(params):
            if k:
                assert z.deflateParams(ctypes.byref(s), level, strategy) in (0, -5)
            s.next_in, s.avail_in = ctypes.addressof(src) + k * step, min(step, len(data) - k * step)
            assert z.deflate(ctypes.byref(s), 0) == 0
        assert z.deflate(ctypes.byref(s), 4) == 1                     # Z_FINISH -> Z_STREAM_END
        return out.raw[:s.total_out]
    finally:
        z.deflateEnd(ctypes.byref(s))


def _zlib_flushes(data, modes):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    step = (len(data) + len(modes)) // (len(modes) + 1)
    out = b""
    for k, m in enumerate(modes):
        out += co.compress(data[k * step:(k + 1) * step]) + co.flush(m)
    return out + co.compress(data[len(modes) * step:]) + co.flush()


@pytest.fixture(scope="module")
def encoder_blocks(tmp_path_factory):
    chunks = _bam_payloads(tmp_path_factory.mktemp("enc"))
    out = {}
    for wbits in range(9, 16):
        for mem in (1, 9):
            blocks = []
            for c in chunks[:3]:
                co = zlib.compressobj(9 if wbits % 2 else 4, zlib.DEFLATED, -wbits, mem)
                blocks.append((dw.bgzf(co.compress(c) + co.flush(), c), c))
            out["zlib_w%d_m%d" % (wbits, mem)] = blocks
    sw = [(1, 0), (9, 0), (6, 1), (2, 3), (9, 2), (4, 0)]          # level, strategy (0 default, 1 filtered, 2 huffman only, 3 rle)
    out["zlib_deflateParams"] = [(dw.bgzf(zlib_switching(c, sw[k % 3:] + sw[:k % 3], memlevel=(1, 8, 9)[k % 3]), c), c) for k, c in enumerate(chunks[:6])]
    fl = [zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH, zlib.Z_BLOCK, zlib.Z_BLOCK, zlib.Z_SYNC_FLUSH]
    out["zlib_flushes"] = [(dw.bgzf(_zlib_flushes(c, fl[k % 2:]), c), c) for k, c in enumerate(chunks[:6])]
    return chunks, out


@pytest.mark.parametrize("variant", VARIANTS)
def test_zlib_at_other_settings(encoder_blocks, variant):
    _chunks, enc = encoder_blocks
    for name, members in enc.items():
        for _b, c in members:
            assert zlib.decompress(ic.payload(_b), -15) == c
        got, status, _ = _inflate([b for b, _c in members], variant, True)
        assert not status.any(), (name, status.tolist())
        assert got == b"".join(c for _b, c in members), name


@pytest.mark.parametrize("variant", VARIANTS)
def test_libdeflate_every_level(encoder_blocks, variant):
    ld = _libdeflate()
    if ld is None:
        pytest.skip("libdeflate.so.0 is not on this machine: the libdeflate leg (levels 1-12) is skipped, the zlib leg runs")
    chunks, _enc = encoder_blocks
    blocks, want = [], []
    for level in range(1, 13):
        for c in chunks[level % 4::4][:3]:
            blocks.append(dw.bgzf(libdeflate_compress(ld, level, c), c))
            want.append(c)
    got, status, _ = _inflate(blocks, variant, True)
    assert not status.any(), status.tolist()
    assert got == b"".join(want)


# ---- malformed blocks (CRC off: the decoders' own checks judge them)

@pytest.mark.parametrize("variant", VARIANTS)
def test_malformed_blocks_are_flagged_and_their_neighbours_exact(variant):
    bad = ic.malformed()
    good = ic.good_blocks(n=len(bad) + 1)
    blocks = [good[0][0]]
    for k, (_name, b) in enumerate(bad):
        blocks += [b, good[k + 1][0]]
    got, status, isize = _inflate(blocks, variant, False)
    dst = np.concatenate([[0], np.cumsum(isize.astype(np.int64))])
    for k in range(len(bad) + 1):
        i = 2 * k
        assert status[i] == 0, (variant, k, status.tolist())
        assert got[dst[i]:dst[i + 1]] == good[k][1], (variant, "neighbour", k)
    flagged = {name: int(status[2 * k + 1]) for k, (name, _b) in enumerate(bad)}
    assert all(flagged.values()), (variant, {n: s for n, s in flagged.items() if not s})
