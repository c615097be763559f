"""svx_bgzf_deflate / svx_bgzf_pack on the device (csrc/svx_deflate.hip) on the cases of tests/deflate_enc_cases.py -- crafted blocks
and every 0xFF00-byte block of the inflated golden BAMs and index-build files -- in ONE launch: every member against zlib
(deflate_enc_cases.check_member), byte for byte against the host program that runs the kernel's phase code
(tools/hostwave/deflate_main.cpp), a second launch, the packed file bytes, and the round trip through the device's own inflater
and CRC32 check."""
import numpy as np
import pytest
import torch

from svision_amd import kernels
from tests import deflate_enc_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def launch(tmp_path_factory):
    """One launch over all blocks -> (cases, files, stream, offsets, members as bytes, stored flags, device tensors slots / member_len)."""
    d = tmp_path_factory.mktemp("deflate_gpu")
    cases, files = dc.crafted(), dc.bam_blocks(d)
    blocks = [c.data for c in cases] + [b for _n, b in files]
    stream, off = dc.layout(blocks)                              # (the first block starts at offset 1 of the stream)
    d_in = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).to(DEV)
    d_off = torch.from_numpy(off.view(np.int64)).to(DEV)
    slots, member_len, stored = kernels.bgzf_deflate(d_in, d_off)
    torch.cuda.synchronize()
    lens = member_len.cpu().numpy()
    host_slots = slots.cpu().numpy()
    members = [host_slots[b, :lens[b]].tobytes() for b in range(len(blocks))]
    return dict(dir=d, cases=cases, files=files, blocks=blocks, d_in=d_in, d_off=d_off, off=off, slots=slots, member_len=member_len,
                members=members, stored=stored.cpu().numpy().tolist())


def test_every_member_against_zlib(launch):
    cases, files, members, stored = launch["cases"], launch["files"], launch["members"], launch["stored"]
    for c, m, s in zip(cases, members, stored):
        assert dc.check_member(m, c.data, c) == bool(s), c.name
    for (name, block), m, s in zip(files, members[len(cases):], stored[len(cases):]):
        assert dc.check_member(m, block, dc.Case(name, block)) == bool(s), name
    by_name = dict(zip((c.name for c in cases), members))
    assert by_name["empty"] == dc.EOF_BLOCK and len(by_name["random_0xFF00"]) == 65311 and len(by_name["equal_0xFF00"]) <= 512
    lengths, distances = set(), set()
    for c, m in zip(cases, members):
        if c.want_token is not None and m[18] & 7 == 3:
            for l, dd in dc.tokens(m[18:-8])[0]:
                lengths.add(l)
                distances.add(dd)
    assert set(dc.LENGTHS) <= lengths and set(dc.DISTANCES) <= distances


def test_the_bytes_are_the_host_program_s(launch):
    cases, files = launch["cases"], launch["files"]
    (want, want_stored), = dc.run_host(dc.build_host(launch["dir"]), launch["dir"], cases, files, 1, 1)
    assert launch["members"] == want and launch["stored"] == want_stored


def test_a_second_launch_gives_the_same_bytes(launch):
    slots, member_len, stored = kernels.bgzf_deflate(launch["d_in"], launch["d_off"])
    lens = member_len.cpu().numpy()
    assert np.array_equal(lens, launch["member_len"].cpu().numpy()) and stored.cpu().numpy().tolist() == launch["stored"]
    host_slots = slots.cpu().numpy()
    assert [host_slots[b, :lens[b]].tobytes() for b in range(len(lens))] == launch["members"]


def test_pack_and_round_trip_on_the_device(launch):
    blocks, members = launch["blocks"], launch["members"]
    total_in = sum(len(b) for b in blocks)
    packed, file_off = kernels.bgzf_pack(launch["slots"], launch["member_len"], total_in + kernels.BGZF_MEMBER_EXTRA * len(blocks))
    file_off = file_off.cpu().numpy()
    want = b"".join(members)
    assert file_off[0] == 0 and np.array_equal(np.diff(file_off), [len(m) for m in members]) and int(file_off[-1]) == len(want)
    data = packed[:len(want)].cpu().numpy()
    assert data.tobytes() == want
    # the device's own reader: svx_bgzf_inflate_fast + svx_bgzf_crc32 on the packed bytes
    src_off, src_len, isize, _coff = kernels.bgzf_block_table(data)
    assert len(src_off) == len(blocks) and isize.tolist() == [len(b) for b in blocks]
    d_comp = torch.zeros((len(want) + 31) // 16 * 16, dtype=torch.uint8, device=DEV)
    d_comp[:len(want)] = packed[:len(want)]
    out, status = kernels.bgzf_inflate(d_comp, src_off, src_len, isize, crc=True)
    assert not status.cpu().numpy().any()
    assert out.cpu().numpy().tobytes() == b"".join(blocks)


def test_a_block_above_0xFF00_bytes_is_refused():
    d_in = torch.zeros(0xFF01 + 10, dtype=torch.uint8, device=DEV)
    d_off = torch.tensor([0, 0xFF01, 0xFF01 + 10], dtype=torch.int64, device=DEV)
    _slots, member_len, _stored = kernels.bgzf_deflate(d_in, d_off)
    assert member_len.cpu().numpy().tolist() == [0, 30]          # 10 zero bytes: a literal + a match of 9 at distance 1 = 3 + 8 + 7 + 5 + 7 bits = 4 bytes, + 26
