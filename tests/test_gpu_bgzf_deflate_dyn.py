"""svx_bgzf_deflate_dyn on the device (csrc/svx_deflate.hip) on the blocks of tests/test_bgzf_deflate_dyn_cpu.py -- the crafted cases of
tests/deflate_enc_cases.py and tests/deflate_dyn_cases.py, every block of the straddling, long and decoy index-build files, the first
eight of each golden BAM -- in ONE launch, beside svx_bgzf_deflate on the same blocks: every member against zlib, the fixed form's
member and an own RFC 1951 decoder (deflate_dyn_cases.check_member), byte for byte against the host program that runs the kernel's
phase code (tools/hostwave/deflate_dyn_main.cpp), a second launch, the packed file bytes through the device's own inflater and CRC32
check, and the two refusals: a block above 0xFF00 bytes, a workspace that is too small."""
import numpy as np
import pytest
import torch

from svision_amd import _lib, kernels
from tests import deflate_enc_cases as dc
from tests import deflate_dyn_cases as dy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _members(slots, member_len):
    lens = member_len.cpu().numpy()
    host_slots = slots.cpu().numpy()
    return [host_slots[b, :lens[b]].tobytes() for b in range(len(lens))]


@pytest.fixture(scope="module")
def launch(tmp_path_factory):
    """One launch of each encoder over all blocks -> cases, file sets, blocks, the members and block types, the fixed encoder's members
    and stored flags, the device tensors."""
    d = tmp_path_factory.mktemp("deflate_dyn_gpu")
    cases, sets = dy.all_cases(), dy.file_sets(d)
    files = [b for _s, blocks in sets for b in blocks]
    blocks = [c.data for c in cases] + files
    stream, off = dc.layout(blocks)                              # (the first block starts at offset 1 of the stream)
    d_in = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).to(DEV)
    d_off = torch.from_numpy(off.view(np.int64)).to(DEV)
    slots, member_len, btype = kernels.bgzf_deflate_dynamic(d_in, d_off)
    f_slots, f_len, f_stored = kernels.bgzf_deflate(d_in, d_off)
    torch.cuda.synchronize()
    return dict(dir=d, cases=cases, sets=sets, files=files, blocks=blocks, d_in=d_in, d_off=d_off, slots=slots, member_len=member_len,
                members=_members(slots, member_len), btype=btype.cpu().numpy().tolist(), fixed=_members(f_slots, f_len),
                stored=f_stored.cpu().numpy().tolist())


def test_every_member_against_zlib_and_the_fixed_encoder(launch):
    cases, members, btype, fixed, stored = launch["cases"], launch["members"], launch["btype"], launch["fixed"], launch["stored"]
    lengths, distances, deepest = set(), set(), 0
    for c, m, t, f, s in zip(cases, members, btype, fixed, stored):
        d = dy.check_member(m, c.data, t, f, c, tokens=True)    # never longer than the fixed encoder's, identical where the type is 0 or 1
        assert (t == 0) == bool(s) or t == 2, c.name
        if c.want_token is not None or getattr(c, "want_tokens", None):
            for l, dd in (d.matches if d is not None else dc.tokens(m[18:-8])[0] if t == 1 else []):
                lengths.add(l)
                distances.add(dd)
    assert set(dc.LENGTHS) <= lengths and set(dc.DISTANCES) <= distances
    at = len(cases)
    for name, blocks in launch["sets"]:
        total = 0
        for k, block in enumerate(blocks):
            d = dy.check_member(members[at], block, btype[at], fixed[at], dc.Case("%s[%d]" % (name, k), block))
            if d is not None:
                deepest = max(deepest, max(d.lit_lens))
            total, at = total + len(members[at]), at + 1
        assert total <= dy.zlib_members(blocks, 1), name
    assert deepest == 15
    by_name = dict(zip((c.name for c in cases), zip(members, btype)))
    assert by_name["empty"] == (dc.EOF_BLOCK, 1) and by_name["tiny_300"][1] == 1 and by_name["random_0xFF00"][1] == 0
    assert all(by_name["fibonacci_%d" % k][1] == 2 for k in range(3)) and set(btype) == {0, 1, 2}


def test_the_bytes_are_the_host_program_s(launch):
    d = launch["dir"]
    (want, want_type), = dy.run_host(dy.build_host(d, "deflate_dyn_main"), d, "dyn_", [c.data for c in launch["cases"]], launch["files"], 1, 1)
    assert launch["btype"] == want_type
    assert launch["members"] == want


def test_a_second_launch_gives_the_same_bytes(launch):
    slots, member_len, btype = kernels.bgzf_deflate_dynamic(launch["d_in"], launch["d_off"])
    assert btype.cpu().numpy().tolist() == launch["btype"]
    assert _members(slots, member_len) == launch["members"]


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
    _slots, member_len, btype = kernels.bgzf_deflate_dynamic(d_in, d_off)
    assert member_len.cpu().numpy().tolist() == [0, 30] and btype.cpu().numpy().tolist() == [0, 1]      # 10 zero bytes: 4 bytes in the fixed code, + 26


def test_a_short_workspace_is_an_error():
    """One byte less than svx_bgzf_deflate_dyn_ws_bytes asks for: SVX_ECAPACITY, nothing launched, nothing written."""
    lib = _lib.load()
    n = 3
    need = int(lib.svx_bgzf_deflate_dyn_ws_bytes(n))
    assert need == n * int(lib.svx_bgzf_deflate_dyn_ws_bytes(1)) and 0 < need <= 4 * n * 0xFF00
    d_in = torch.full((3000,), 7, dtype=torch.uint8, device=DEV)
    d_off = torch.tensor([0, 1000, 2000, 3000], dtype=torch.int64, device=DEV)
    slots = torch.full((n, kernels.BGZF_SLOT), 0x5A, dtype=torch.uint8, device=DEV)
    member_len = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    btype = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    args = (d_in.data_ptr(), d_off.data_ptr(), n, slots.data_ptr(), member_len.data_ptr(), btype.data_ptr(), ws.data_ptr())
    assert lib.svx_bgzf_deflate_dyn(*args, need - 1, kernels._stream_ptr(torch.device(DEV))) == -2           # SVX_ECAPACITY
    torch.cuda.synchronize()
    assert member_len.cpu().numpy().tolist() == [-1] * n and btype.cpu().numpy().tolist() == [-1] * n
    assert bool((slots == 0x5A).all()) and not bool(ws.any())
    assert lib.svx_bgzf_deflate_dyn(*args, need, kernels._stream_ptr(torch.device(DEV))) == 0
    torch.cuda.synchronize()
    assert (member_len.cpu().numpy() > 26).all()
