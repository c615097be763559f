"""svx_bgzf_crc32 (csrc/svx_crc.hip) called directly (-m gpu), against zlib.crc32: blocks of chosen lengths laid end to end
in d_out -- the kernel's special cases are keyed on len mod 4 and dst_off mod 4: blocks under four bytes, the dword that
straddles the start of the data, the initial-value mask, lengths up to 65,536 --, d_comp holding nothing but their 8-byte
footers.  A correct footer leaves the status alone, any single flipped bit -- in the footer or in the data -- gives
SVX_INFLATE_BAD_CRC (9).  tests/test_walkcases_cpu.py checks that the block table holds all 16 classes at both ends."""
import zlib

import numpy as np
import pytest
import torch

from svision_amd import _lib, kernels
from tests import walkcases as wc

pytestmark = pytest.mark.gpu
BAD_CRC = 9
SENTINEL = 0xA5A5A5A5


def _dev():
    return torch.device("cuda:0")


class Blocks:
    """``data`` cut into blocks of ``lengths`` on the device, with the footers zlib gives them."""

    def __init__(self, data, lengths):
        self.data, self.lengths = data, list(lengths)
        self.off = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        assert int(self.off[-1]) == data.size
        self.crc = np.asarray([zlib.crc32(data[a:b]) for a, b in zip(self.off, self.off[1:])], np.uint32)
        self.d_out = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(_dev())
        self.d_off = torch.from_numpy(self.off).to(_dev())
        n = len(self.lengths)
        self.d_src_off = torch.arange(0, 8 * n, 8, dtype=torch.int64, device=_dev())
        self.d_src_len = torch.zeros(n, dtype=torch.int32, device=_dev())

    def run(self, crc=None, d_out=None, status=None, n_blocks=None):
        """-> the statuses of the first ``n_blocks`` blocks; the entries behind them must not have been touched."""
        n = len(self.lengths) if n_blocks is None else n_blocks
        foot = np.zeros((len(self.lengths), 2), np.uint32)
        foot[:, 0], foot[:, 1] = self.crc if crc is None else crc, np.asarray(self.lengths, np.uint32)
        d_comp = torch.from_numpy(foot.view(np.uint8).reshape(-1).copy()).to(_dev())
        h_status = np.full(n + 8, SENTINEL, np.uint32)
        h_status[:n] = 0 if status is None else status
        d_status = torch.from_numpy(h_status.view(np.int32).copy()).to(_dev())
        _lib.check(_lib.load().svx_bgzf_crc32((self.d_out if d_out is None else d_out).data_ptr(), self.d_off.data_ptr(), d_comp.data_ptr(), self.d_src_off.data_ptr(),
                                              self.d_src_len.data_ptr(), n, d_status.data_ptr(), kernels._stream_ptr(_dev())), "svx_bgzf_crc32")
        torch.cuda.synchronize()
        got = d_status.cpu().numpy().view(np.uint32)
        assert (got[n:] == SENTINEL).all()
        return got[:n]


@pytest.fixture(scope="module")
def table():
    lengths = wc.crc_lengths()
    rng = np.random.default_rng(21)
    return Blocks(rng.integers(0, 256, sum(lengths), dtype=np.uint8), lengths)


def test_correct_footers_leave_every_status_alone(table):
    got = table.run()
    assert not got.any(), [table.lengths[b] for b in np.flatnonzero(got)][:10]


def test_a_flipped_footer_bit(table):
    rng = np.random.default_rng(22)
    crc = table.crc ^ (np.uint32(1) << rng.integers(0, 32, table.crc.size).astype(np.uint32))
    got = table.run(crc=crc)
    assert (got == BAD_CRC).all(), [table.lengths[b] for b in np.flatnonzero(got != BAD_CRC)][:10]


@pytest.mark.parametrize("where", ["first", "byte3", "byte4", "last", "random"])
def test_a_flipped_data_bit(table, where):
    """One bit of every block that has the byte: the first byte, byte 3 and byte 4 (the two sides of the first dword, whose
    complement stands for the initial value), the last byte, one anywhere."""
    rng = np.random.default_rng(23)
    lengths = np.asarray(table.lengths, np.int64)
    at = {"first": np.zeros_like(lengths), "byte3": np.full_like(lengths, 3), "byte4": np.full_like(lengths, 4), "last": lengths - 1,
          "random": (rng.random(lengths.size) * lengths).astype(np.int64)}[where]
    has = (at >= 0) & (at < lengths)
    assert has.sum() >= lengths.size - 5
    idx = torch.from_numpy((table.off[:-1] + at)[has]).to(_dev())
    bits = torch.from_numpy((1 << rng.integers(0, 8, int(has.sum()))).astype(np.uint8)).to(_dev())
    d_out = table.d_out.clone()
    d_out[idx] = d_out[idx] ^ bits
    got = table.run(d_out=d_out)
    assert np.array_equal(got, np.where(has, BAD_CRC, 0)), [table.lengths[b] for b in np.flatnonzero(got != np.where(has, BAD_CRC, 0))][:10]


def test_every_bit_of_a_260_byte_block():
    rng = np.random.default_rng(24)
    block = rng.integers(0, 256, 260, dtype=np.uint8)
    copies = np.tile(block, (2081, 1))
    for bit in range(2080):
        copies[bit, bit >> 3] ^= 1 << (bit & 7)
    lead = rng.integers(0, 256, 3, dtype=np.uint8)             # (the blocks do not begin on a multiple of 4)
    b = Blocks(np.concatenate([lead, copies.reshape(-1)]), [3] + [260] * 2081)
    want = np.full(2082, zlib.crc32(block), np.uint32)
    want[0] = zlib.crc32(lead)
    got = b.run(crc=want)
    assert got[0] == 0 and got[-1] == 0 and (got[1:-1] == BAD_CRC).all(), np.flatnonzero(got[1:-1] != BAD_CRC)[:10]


def test_a_status_already_set_stays_and_an_oversized_block_is_refused():
    rng = np.random.default_rng(25)
    lengths = [100, 65537, 100, 7, 300]
    b = Blocks(rng.integers(0, 256, sum(lengths), dtype=np.uint8), lengths)
    assert b.run().tolist() == [0, BAD_CRC, 0, 0, 0]            # a gap of 65,537 in dst_off is no BGZF block, whatever its footer says
    wrong = b.crc ^ np.uint32(0x10)
    assert b.run(crc=wrong).tolist() == [BAD_CRC] * 5
    assert b.run(crc=wrong, status=[5, 5, 0, 5, 0]).tolist() == [5, 5, BAD_CRC, 5, BAD_CRC]
    assert b.run(status=[5, 5, 0, 5, 0]).tolist() == [5, 5, 0, 5, 0]


@pytest.mark.parametrize("n_blocks", [1, 3, 4, 5, 1027])
def test_block_counts_around_the_workgroup(n_blocks):
    """Four waves, a block each, per workgroup: a ragged last group writes no status behind the last block."""
    rng = np.random.default_rng(26)
    lengths = rng.integers(0, 200, 1027).tolist()
    b = Blocks(rng.integers(0, 256, sum(lengths), dtype=np.uint8), lengths)
    wrong = np.arange(1027) % 3 == 1
    got = b.run(crc=np.where(wrong, b.crc ^ np.uint32(1 << 31), b.crc), n_blocks=n_blocks)
    assert np.array_equal(got, np.where(wrong[:n_blocks], BAD_CRC, 0))
