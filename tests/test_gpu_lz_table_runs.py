"""bgzf_lz_table_kernel ("fast-table": csrc/svx_lz_table.hip) on long literal runs and long matches, from explicit tokens
(tests/lz_run_cases.py) == zlib, byte for byte: runs of 15 .. 600 literals, matches of 15 .. 258 bytes at distance 1, distance =
length and distance 32,768, a wave whose 64 sequences are all long, one long sequence in lane 0 / in lane 63 of a wave, long
sequences on both sides of a batch border (sequences 1,023 and 1,024), blocks of exactly 0xFF00 bytes that end in a long run, a
stored block in front of a compressed one -- every block once with its output at an address 0 mod 16 and once at 15 mod 16 -- and
a long match that starts in front of its block: flagged, its neighbours exact."""
import numpy as np
import pytest
import torch

from svision_amd import kernels
from tests import lz_run_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return rc.build()


@pytest.mark.parametrize("phase", [0, 15])
def test_long_runs_decode_like_zlib_and_the_malformed_one_is_flagged(cases, phase):
    launch = rc.at_phase(cases, phase)
    raw = np.frombuffer(b"".join(b for b, _d, _s in launch), np.uint8)
    src_off, src_len, isize, _blk = kernels.bgzf_block_table(raw)
    assert len(src_off) == len(launch)
    padded = np.zeros((raw.size + 31) // 16 * 16, np.uint8)
    padded[:raw.size] = raw
    out, status = kernels.bgzf_inflate(torch.from_numpy(padded).cuda(), src_off, src_len, isize, wave="fast-table", crc=False)
    got, status = out.cpu().numpy().tobytes(), status.cpu().numpy()
    assert status.tolist() == [s for _b, _d, s in launch]
    dst = np.concatenate([[0], np.cumsum(isize.astype(np.int64))])
    names = {2 * k + 1: c.name for k, c in enumerate(cases)}
    for k, (_b, want, _s) in enumerate(launch):
        if want is not None:
            assert dst[k + 1] - dst[k] == len(want)
            assert got[dst[k]:dst[k + 1]] == want, (names.get(k, "filler"), k)
        if k in names:
            assert dst[k] % 16 == phase
