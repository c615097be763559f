"""The native staging reader inside the device decoder (ingest_gpu._Pipeline: svx_stage_open / svx_stage_group / svx_stage_close)
with slots of 128 KB and 256 KB and groups of about 1 MB, so that a 5 MB file takes a dozen slots per group, the ring wraps and
the read-ahead runs from one group into the next: the bytes that reach the device are the file's, the decoded tables are those
of the Python loop (SVX_STAGE_READER=py) and of the host engine, and a damaged file or an abandoned run ends with an error value
or a return, in time, with the ring released and no thread left."""
import shutil
import threading
import time

import numpy as np
import pytest
import torch

import svision_amd.ingest_gpu as ig
from svision_amd.io import bam

pytestmark = pytest.mark.gpu
FIELDS = ("tid", "pos", "flag", "mapq", "l_seq", "name_id", "cigar", "cig_off")
LIMIT_S = 20.0                              # "in time": the runs below take a fraction of a second; the pipeline's own waits are 0.2 s and 10 s


@pytest.fixture(scope="module")
def hifi(tmp_path_factory):
    """The 400 kb synthetic HiFi BAM of the inflate tests (192 blocks) -> (path, header, the file's bytes)."""
    from svision_amd import synth
    table, _g, _ = synth.simulate(synth.SimConfig(contigs=[("c1", 400_000)], coverage=20, seed=4), with_genome=False)
    seg = bam.encode_reference_segment(table, seq="random", seed=1)
    path = str(tmp_path_factory.mktemp("stage") / "hifi.bam")
    bam.write_bam_segments(path, table.references, table.lengths, [seg])
    return path, bam.read_bam_header(path), np.fromfile(path, np.uint8)


@pytest.fixture(autouse=True)
def _small_slots_and_groups():
    saved = {k: getattr(ig, k) for k in ("STAGE_BYTES", "FIRST_GROUP_BYTES", "PIPE_GROUP_BYTES", "LARGE_GROUP_BYTES")}
    ig.FIRST_GROUP_BYTES = ig.PIPE_GROUP_BYTES = ig.LARGE_GROUP_BYTES = 1 << 20
    yield
    for k, v in saved.items():
        setattr(ig, k, v)


def _decoder(path, head):
    return ig.DeviceDecoder(path, path + ".bai", head.references, head.lengths, head.header_text, "cuda:0", threads=3)


def _slices(dec):
    """The reference in slices of one 50 kb window + 16 kb margins each, ~1.2 MB of file: eight units, a group each (the margin is
    given: nothing is estimated from the file, which one test damages)."""
    return dec.plan_units([0], windows_of=lambda _t: [(s, s + 50_000) for s in range(0, 400_000, 50_000)], margin=16384, slice_bytes=1 << 20,
                          min_span_margins=0)


def _tables(dec, units):
    out = []
    for unit, finish, _arrays in dec.units_pipelined(units):
        if finish is None:
            out.append((repr(unit), None))
            continue
        tb = finish()
        ig.spill_cigar(tb)
        out.append((repr(unit), {f: np.asarray(getattr(tb, f)).copy() for f in FIELDS}, [tb.names[i] for i in tb.name_id]))
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0] and (x[1] is None) == (y[1] is None)
        if x[1] is not None:
            for f in FIELDS:
                assert np.array_equal(x[1][f], y[1][f]), (x[0], f)
            assert x[2] == y[2]


def _quiet(before):
    """The pipeline's daemon threads end on their own once the run is over: wait for them, at most a few seconds."""
    t_end = time.time() + 5
    while threading.active_count() > before and time.time() < t_end:
        time.sleep(0.01)
    assert threading.active_count() <= before, [t.name for t in threading.enumerate()]
    assert not ig._StagingRing._busy


@pytest.mark.parametrize("stage_bytes", [128 << 10, 256 << 10])
def test_the_bytes_on_the_device_are_the_files(hifi, monkeypatch, stage_bytes):
    path, head, raw = hifi
    monkeypatch.delenv("SVX_STAGE_READER", raising=False)
    ig.STAGE_BYTES = stage_bytes
    dec = _decoder(path, head)
    pipe = ig._Pipeline(dec, _slices(dec), 2)
    assert pipe.native and len(pipe.groups) >= 3
    slots = 0
    try:
        pipe.open_stage()
        for g, (c0, c1) in zip(pipe.groups, pipe.ranges):
            grp = pipe.read_group(g)
            grp.copied.synchronize()
            tv = grp.tab.numpy()
            nb = grp.n_blocks
            used = int(tv[nb - 1] + tv[2 * nb - 1]) + 8                   # the end of the last block's footer
            assert c1 - c0 - 65536 - 64 <= used <= c1 - c0
            assert np.array_equal(grp.d_comp[:used].cpu().numpy(), raw[c0:c0 + used]), (c0, c1)
            slots += -(-(c1 - c0) // (stage_bytes - 65536))
        assert slots > 3 * len(pipe.ring.slots)                            # the ring wrapped, several times
    finally:
        pipe.copy_stream.synchronize()
        if pipe.stage:
            pipe.lib.svx_stage_close(pipe.stage)
        pipe.ring.release()


@pytest.mark.parametrize("stage_bytes", [128 << 10, 256 << 10])
def test_tables_equal_the_python_loops_and_the_host_engines(hifi, monkeypatch, stage_bytes):
    path, head, _raw = hifi
    ig.STAGE_BYTES = stage_bytes
    got = {}
    for reader in ("native", "py"):
        monkeypatch.setenv("SVX_STAGE_READER", reader)
        dec = _decoder(path, head)
        got[reader] = _tables(dec, _slices(dec)), _tables(dec, dec.whole_units([0]))
        assert dec.stats["blocks"] > 192                                  # (the slices overlap by their margins)
    assert len(got["native"][0]) >= 3
    _same(got["native"][0], got["py"][0])
    _same(got["native"][1], got["py"][1])
    host = bam.read_bam(path, tids=[0])
    whole = got["native"][1]
    assert len(whole) == 1
    for f in FIELDS:
        assert np.array_equal(whole[0][1][f], np.asarray(getattr(host, f))), f
    assert whole[0][2] == [host.names[i] for i in host.name_id]


def test_a_damaged_file_raises_in_time_and_the_next_run_works(hifi, monkeypatch, tmp_path):
    path, head, raw = hifi
    monkeypatch.delenv("SVX_STAGE_READER", raising=False)
    ig.STAGE_BYTES = 128 << 10
    blk = ig.kernels.bgzf_block_table(raw)[3]
    at = int(blk[blk.size * 2 // 3])                                      # a block's magic two thirds into the file: a later group, a later slot
    bad = raw.copy()
    bad[at:at + 4] = 0
    bad_path = str(tmp_path / "damaged.bam")
    bad.tofile(bad_path)
    shutil.copy(path + ".bai", bad_path + ".bai")
    before = threading.active_count()
    dec = _decoder(bad_path, head)
    t0 = time.time()
    with pytest.raises(ig.DeviceIngestError) as err:
        _tables(dec, _slices(dec))
    assert time.time() - t0 < LIMIT_S
    assert err.value.tids == [0] and "no BGZF block at file offset %d" % at in str(err.value)
    _quiet(before)
    good = _decoder(path, head)
    assert len(_tables(good, _slices(good))) >= 3
    _quiet(before)


def test_an_abandoned_run_returns_in_time_and_the_next_run_works(hifi, monkeypatch):
    path, head, _raw = hifi
    monkeypatch.delenv("SVX_STAGE_READER", raising=False)
    ig.STAGE_BYTES = 128 << 10
    before = threading.active_count()
    dec = _decoder(path, head)
    units = _slices(dec)
    gen = dec.units_pipelined(units)
    first = next(gen)
    assert first[0] is units[0]
    t0 = time.time()
    gen.close()
    assert time.time() - t0 < LIMIT_S
    _quiet(before)
    torch.cuda.synchronize()
    again = _decoder(path, head)
    assert len(_tables(again, _slices(again))) == len(units)
    _quiet(before)
