"""svx_record_tags_measure / svx_record_tags_write on the device (svision_amd/csrc/svx_recsort.hip, kernels.record_tags_*): the
crafted streams of tests/tagcases.py, each under its drop list and under the complementary keep list.  Lengths, bytes and status must
equal the Python walker's AND the stand-alone host program's (tools/hostwave/tags_main.cpp, the same wave routines); the destination
lies between two guard bands of a pattern that must survive, at every alignment; a second run gives the same bytes."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from svision_amd import _lib, kernels
from tests import tagcases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, PATTERN = 64, 0xA5


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host program"
    out = str(tmp_path_factory.mktemp("hostwave") / "tags_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-o", out, os.path.join(ROOT, "tools", "hostwave", "tags_main.cpp")])
    return out


def _launch(data, off, mode, tags, align):
    """measure, an exclusive sum on the device, write into a destination that starts GUARD + align bytes into its buffer ->
    (lengths, the whole buffer, status of measure, status of write)."""
    d_bytes, d_off = torch.from_numpy(data).to(DEV), torch.from_numpy(off).to(DEV)
    table = kernels.tags_table(tags, mode == "keep", DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    d_len = kernels.record_tags_measure(d_bytes, d_off, table, status)
    measured = int(status.item())
    d_new_off = torch.full((off.size,), GUARD + align, dtype=torch.int64, device=DEV)
    d_new_off[1:] += torch.cumsum(d_len, 0)
    out = torch.full((int(d_new_off[-1].item()) + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    status.zero_()
    assert kernels.record_tags_write(d_bytes, d_off, table, d_new_off, out, status) is out
    return d_len.cpu().numpy(), out.cpu().numpy(), measured, int(status.item())


def _check(program, path, records, drop, skew, status=None):
    data, off = tagcases.place(records, skew)
    align = (3 * skew + 1) % 4                                  # every alignment of the destination, none equal to the source's
    at = GUARD + align
    for mode, tags in tagcases.filters(records, drop):
        want, want_len, want_status = tagcases.expected(data, off, mode, tags)
        host = tagcases.run_host(program, path, data, off, mode, tags)
        got_len, buf, measured, written = _launch(data, off, mode, tags, align)
        assert np.array_equal(got_len, want_len) and np.array_equal(got_len, host[1]), (mode, tags)
        assert buf.size == at + want.size + GUARD and (buf[:at] == PATTERN).all() and (buf[at + want.size:] == PATTERN).all()
        assert np.array_equal(buf[at:at + want.size], want) and np.array_equal(host[0], want), (mode, tags)
        assert measured == written == want_status == host[2] == host[3] and (status is None or want_status == status)
        again = _launch(data, off, mode, tags, align)
        assert np.array_equal(again[1], buf) and np.array_equal(again[0], got_len)
    return want_len, off


@pytest.mark.parametrize("n", tagcases.COUNTS)
def test_record_counts_at_every_skew(program, tmp_path, n):
    for skew in range(4):
        new_len, off = _check(program, str(tmp_path / "case.bin"), tagcases.mixed(n, seed=skew), tagcases.DROP, skew, status=0)
        assert n < 12 or (new_len < np.diff(off)).any() and (new_len == np.diff(off)).any()


@pytest.mark.parametrize("case", tagcases.shape_cases(), ids=lambda c: c[0])
def test_shapes(program, tmp_path, case):
    name, records, drop = case
    bad = name.startswith("malformed")
    for skew in range(4):
        new_len, off = _check(program, str(tmp_path / "case.bin"), records, drop, skew, status=int(bad))
    if bad:
        which = 2 if "at the end" in name else 1
        assert new_len[which] == off[which + 1] - off[which] and all(new_len[r] < off[r + 1] - off[r] for r in range(3) if r != which)


def test_offsets_that_do_not_fit():
    """d_new_off that gives a record another length than its walk: that record is not written -- its destination keeps the pattern
    -- and the status says so; the others are written."""
    records = tagcases.mixed(9)
    data, off = tagcases.place(records, 1)
    want, want_len, _status = tagcases.expected(data, off, "drop", tagcases.DROP)
    d_bytes, d_off, table = torch.from_numpy(data).to(DEV), torch.from_numpy(off).to(DEV), kernels.tags_table(tagcases.DROP, False, DEV)
    at = np.concatenate([[0], np.cumsum(want_len)])
    for grow in (1, -1):                                        # record 4 a byte too long, a byte too short
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        new_off = at.copy()
        new_off[5:] += grow
        out = torch.full((int(new_off[-1]),), PATTERN, dtype=torch.uint8, device=DEV)
        kernels.record_tags_write(d_bytes, d_off, table, torch.from_numpy(new_off).to(DEV), out, status)
        got = out.cpu().numpy()
        assert int(status.item()) == 1 and (got[new_off[4]:new_off[5]] == PATTERN).all()
        for r in (0, 3, 5, 8):
            assert np.array_equal(got[new_off[r]:new_off[r] + want_len[r]], want[at[r]:at[r + 1]])
    # the offsets of the walk: status 0
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((int(at[-1]),), PATTERN, dtype=torch.uint8, device=DEV)
    kernels.record_tags_write(d_bytes, d_off, table, torch.from_numpy(at).to(DEV), out, status)
    assert int(status.item()) == 0 and np.array_equal(out.cpu().numpy(), want)


def test_arguments():
    data, off = tagcases.place(tagcases.mixed(5), 0)
    d = lambda a: torch.from_numpy(a).to(DEV)
    table, status = kernels.tags_table(("fi",), False, DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    assert table.dtype == torch.int32 and table.shape == (2048,) and np.array_equal(table.cpu().numpy(), tagcases.bitmap("drop", ("fi",)))
    out = torch.zeros(data.size + 64, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_measure(torch.from_numpy(data), d(off), table, status)              # a CPU tensor
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_measure(d(data), torch.from_numpy(off), table, status)
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_measure(d(data), d(off), table.cpu(), status)
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_measure(d(data), d(off).to(torch.int32), table, status)             # wrong dtypes
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_measure(d(data).to(torch.int8), d(off), table, status)
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_measure(d(data), d(off), table, status.to(torch.int64))
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_measure(d(data), d(off), table[:-1], status)                        # a table of another size
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_measure(d(data), d(off), table.view(torch.uint8), status)
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_measure(d(data), d(off[:0].copy()), table, status)                   # offsets are [n + 1]: at least one
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_write(d(data), d(off), table, d(off[:-1].copy()), out, status)       # offsets of the wrong length
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_write(d(data), d(off), table, d(off).to(torch.int32), out, status)
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_write(d(data), d(off), table, d(off), out.cpu(), status)
    with pytest.raises(_lib.SvxError):
        kernels.record_tags_write(d(data), d(off), table, d(off), out.to(torch.int16), status)
    with pytest.raises(_lib.SvxError):
        kernels.tags_table(("CG",), False, DEV)
    # no record: no launch, no length
    assert kernels.record_tags_measure(d(data), d(off[:1].copy()), table, status).numel() == 0
