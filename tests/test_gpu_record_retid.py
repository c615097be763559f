"""svx_record_retid on the device (svision_amd/csrc/svx_recsort.hip, kernels.record_retid): the crafted streams of tests/retidcases.py
-- the cases of the host program in tests/test_sort_merge_cpu.py -- must come out as the struct.pack_into model says and as the host
program leaves them, byte for byte: sentinels, keys and status.  Sizes around the wave and the workgroup, and one launch with more
records than the grid has lanes."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import retidcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IN = 7


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_path_factory.mktemp("hostwave") / "retid_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-o", out, os.path.join(ROOT, "tools", "hostwave", "retid_main.cpp")])
    return out


def _launch(data, off, table, key):
    from svision_amd import kernels
    d_bytes, d_off, d_map = (torch.from_numpy(a.copy()).to(DEV) for a in (data, off, np.asarray(table, np.int32)))
    d_key = None if key is None else torch.from_numpy(key.copy()).to(DEV)
    d_status = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert kernels.record_retid(d_bytes, d_off, d_map, d_key, d_status) is d_bytes
    return d_bytes.cpu().numpy(), None if d_key is None else d_key.cpu().numpy(), int(d_status.item()), (d_bytes, d_off, d_key)


@pytest.mark.parametrize("bad", [False, True], ids=["inside", "outside"])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 300, 3 * 256 + 1])
def test_against_the_model_and_the_host_program(program, tmp_path, n, bad):
    table = retidcases.table(N_IN)
    for skew in range(4):
        data, off, key = retidcases.stream(n, skew, N_IN, bad=bad)
        for with_key in (True, False):
            k = key if with_key else None
            want = retidcases.expected(data, off, table, k)
            got = _launch(data, off, table, k)
            assert np.array_equal(got[0], want[0]), (n, skew, with_key)
            assert (got[1] is None and want[1] is None) or np.array_equal(got[1], want[1])
            assert got[2] == want[2] == int(bad and n > 1)
        if skew == n % 4:                                       # the host program's bytes: one skew a size
            host, device = retidcases.run_host(program, str(tmp_path / "case.bin"), data, off, table, key), _launch(data, off, table, key)
            assert np.array_equal(host[0], device[0]) and np.array_equal(host[1], device[1]) and host[2] == device[2]


def test_identity_and_inverse():
    """The identity table changes nothing; a permutation and then its inverse on the same buffer restore the input."""
    data, off, key = retidcases.stream(3 * 256 + 1, 3, N_IN)
    got = _launch(data, off, np.arange(N_IN, dtype=np.int32), key)
    assert np.array_equal(got[0], data) and np.array_equal(got[1], key) and got[2] == 0
    from svision_amd import kernels
    perm = np.random.default_rng(3).permutation(N_IN).astype(np.int32)
    inverse = np.empty(N_IN, np.int32)
    inverse[perm] = np.arange(N_IN, dtype=np.int32)
    once = _launch(data, off, perm, key)
    want = retidcases.expected(data, off, perm, key)
    assert np.array_equal(once[0], want[0]) and not np.array_equal(once[0], data) and once[2] == 0
    d_bytes, d_off, d_key = once[3]
    d_status = torch.zeros(1, dtype=torch.int32, device=DEV)
    kernels.record_retid(d_bytes, d_off, torch.from_numpy(inverse).to(DEV), d_key, d_status)
    assert np.array_equal(d_bytes.cpu().numpy(), data) and np.array_equal(d_key.cpu().numpy(), key) and int(d_status.item()) == 0


def test_more_records_than_lanes():
    """2,048 x 256 + 5 records of 36 bytes at skew 1: the grid-stride loop takes a second turn.  The model is vectorised here: the same
    rule on the two columns of an [n, 36] byte matrix."""
    n, skew = 2048 * 256 + 5, 1
    rng = np.random.default_rng(9)
    table = retidcases.table(N_IN, seed=1)
    rows = rng.integers(0, 256, (n, 36), dtype=np.uint8)
    tid, nxt = rng.integers(-1, N_IN, n).astype("<i4"), rng.integers(-1, N_IN, n).astype("<i4")
    rows[:, 0:4] = np.full(n, 32, "<i4").view(np.uint8).reshape(n, 4)
    rows[:, 4:8], rows[:, 24:28] = tid.view(np.uint8).reshape(n, 4), nxt.view(np.uint8).reshape(n, 4)
    data = np.concatenate([np.full(skew, 0xA5, np.uint8), rows.reshape(-1)])
    off = skew + 36 * np.arange(n, dtype=np.int64)
    want = rows.copy()
    for col, v in ((4, tid), (24, nxt)):
        want[:, col:col + 4] = np.where(v < 0, v, table[np.maximum(v, 0)]).astype("<i4").view(np.uint8).reshape(n, 4)
    got = _launch(data, off, table, tid.astype(np.int32))
    assert np.array_equal(got[0][skew:].reshape(n, 36), want) and got[0][0] == 0xA5 and got[2] == 0
    assert np.array_equal(got[1], np.where(tid < 0, tid, table[np.maximum(tid, 0)]))
    # one field outside in the last record, which only the loop's second turn reaches
    data[int(off[-1]) + 24:int(off[-1]) + 28] = np.asarray([N_IN], "<i4").view(np.uint8)
    got = _launch(data, off, table, None)
    want[-1] = data[int(off[-1]):]
    assert np.array_equal(got[0][skew:].reshape(n, 36), want) and got[2] == 1


def test_arguments():
    from svision_amd import _lib, kernels
    data, off, key = retidcases.stream(5, 0, N_IN)
    d = lambda a: torch.from_numpy(a).to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.SvxError):
        kernels.record_retid(d(data), d(off).to(torch.int32), d(retidcases.table(N_IN)), None, status)
    with pytest.raises(_lib.SvxError):
        kernels.record_retid(d(data), d(off), d(retidcases.table(N_IN)), d(key[:3].copy()), status)
    with pytest.raises(_lib.SvxError):
        kernels.record_retid(torch.from_numpy(data), d(off), d(retidcases.table(N_IN)), None, status)
    assert _lib.load().svx_version() == 420
