"""svx_bgzf_inflate_fast_lz with lz_kernel 3 ("fast-table": csrc/svx_lz_table.hip, a block's LZ77 copies by pointer doubling in
a table in LDS, a workgroup per block) == zlib, byte for byte: the catalogue of streams zlib never writes, the malformed
members flagged with the codes of "fast-wave", blocks above 0xFF00 bytes handed over inside the same launch, more workgroups
than the chip has CUs, the golden BAMs and a synthetic HiFi one, and the same launch twice."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from svision_amd import kernels
from svision_amd.io import bam
from tests import helpers
from tests import inflate_cases as ic

pytestmark = pytest.mark.gpu

VARIANT = "fast-table"


def _block(payload, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    cdata = co.compress(payload) + co.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(cdata) + 25) + cdata
            + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


def _inflate(blocks, variant=VARIANT, crc=True):
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
def test_catalogue_decodes_exactly(catalogue, crc):
    for group, members in catalogue.items():                    # a launch per group: "phase" and "slot" depend on the layout
        got, status, _isize = _inflate([b for b, _d in members], crc=crc)
        assert not status.any(), (group, status.tolist())
        assert got == b"".join(d for _b, d in members), group


def test_malformed_blocks_are_flagged_like_fast_wave_and_their_neighbours_exact():
    bad = ic.malformed()
    good = ic.good_blocks(n=len(bad) + 1)
    blocks = [good[0][0]]
    for k, (_name, b) in enumerate(bad):
        blocks += [b, good[k + 1][0]]
    got, status, isize = _inflate(blocks, crc=False)
    _got, wave_status, _ = _inflate(blocks, variant="fast-wave", crc=False)
    dst = np.concatenate([[0], np.cumsum(isize.astype(np.int64))])
    for k in range(len(bad) + 1):
        assert status[2 * k] == 0, (k, status.tolist())
        assert got[dst[2 * k]:dst[2 * k + 1]] == good[k][1], ("neighbour", k)
    assert all(status[1::2]), [n for (n, _b), s in zip(bad, status[1::2]) if not s]
    assert status.tolist() == wave_status.tolist()


def test_blocks_above_0xff00_bytes_are_handed_over_inside_the_launch():
    rng = np.random.default_rng(12)
    sizes = [0xFF00, 0xFF01, 0xFFFF, 1, 0xFF00 - 1, 0xFF80, 0, 0xFF00, 0xFFFE, 33]
    payloads = [bytes(rng.integers(65, 69, n, dtype=np.uint8)) for n in sizes]
    payloads[0] = bytes(0xFF00)                                  # the deepest chain a block can hold: one value, distance 1
    got, status, _ = _inflate([_block(p, level=(1, 6, 9)[k % 3]) for k, p in enumerate(payloads)])
    assert not status.any(), status.tolist()
    assert got == b"".join(payloads)


def test_more_workgroups_than_the_chip_holds_at_once():
    rng = np.random.default_rng(13)
    payloads = [bytes(rng.integers(65, 70, int(rng.integers(0, 400)), dtype=np.uint8)) * int(rng.integers(1, 4)) for _ in range(600)]
    got, status, _ = _inflate([_block(p, level=(1, 6)[k % 2]) for k, p in enumerate(payloads)])
    assert not status.any()
    assert got == b"".join(payloads)


@pytest.fixture(scope="module")
def bam_files(tmp_path_factory):
    from svision_amd import synth
    table, _g, _ = synth.simulate(synth.SimConfig(contigs=[("c1", 400_000)], coverage=20, seed=4), with_genome=False)
    seg = bam.encode_reference_segment(table, seq="random", seed=1)          # libdeflate level 1 blocks, realistic SEQ / QUAL
    p = str(tmp_path_factory.mktemp("table") / "hifi.bam")
    bam.write_bam_segments(p, table.references, table.lengths, [seg])
    paths = [os.path.join(helpers.GOLDEN, n) for n in ("collect_small.bam", "ont_small.bam", "hash_collect.bam")] + [p]
    return [(path, open(path, "rb").read()) for path in paths]


def _inflate_file(raw):
    r = np.frombuffer(raw, np.uint8)
    src_off, src_len, isize, _blk = kernels.bgzf_block_table(r)
    padded = np.zeros((r.size + 31) // 16 * 16, np.uint8)
    padded[:r.size] = r
    out, status = kernels.bgzf_inflate(torch.from_numpy(padded).cuda(), src_off, src_len, isize, wave=VARIANT)
    return out.cpu().numpy().tobytes(), status.cpu().numpy()


def test_golden_and_synthetic_bams_inflate_like_zlib(bam_files):
    for path, raw in bam_files:
        got, status = _inflate_file(raw)
        assert not status.any(), path
        assert got == bam.bgzf_decompress(raw), path


def test_the_same_launch_twice_gives_the_same_bytes(bam_files):
    _path, raw = bam_files[-1]
    a, sa = _inflate_file(raw)
    b, sb = _inflate_file(raw)
    assert a == b and sa.tolist() == sb.tolist() and not sa.any()
