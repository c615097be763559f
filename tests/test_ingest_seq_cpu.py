"""The lazy read bases of a device-decoded table (ingest_gpu.LazySeq) without a GPU: a reader in the owner process waits for
the spill's event, a helper process waits for the slot's ``seq.ready`` flag, and AlignmentTable.query_sequence / subset give on
the lazy form what they give on the eager one.  (The device side: tests/test_gpu_ingest_seq.py.)"""
import os
import threading
import time

import numpy as np
import pytest

from svision_amd import ingest, synth
from svision_amd.io import bam


@pytest.fixture(scope="module")
def eager():
    cfg = synth.SimConfig(contigs=[("c1", 60_000), ("c2", 40_000)], coverage=6, read_len_mean=3000, read_len_sd=500, sv_spacing=9000,
                          sv_min_gap=5000, sv_max=800, seed=4)
    table, _genome, _ = synth.simulate(cfg, with_seq=True)
    assert sum(table.query_sequence(i) is not None for i in range(len(table))) > 20
    return table


def _lazy_twin(table, lazy):
    return bam.AlignmentTable(table.references, table.lengths, table.tid, table.pos, table.flag, table.mapq, table.l_seq, table.name_id,
                              table.names, table.cigar, table.cig_off, table.header_text, lazy, table.seq_off)


def test_lazy_bases_in_the_owner_process_wait_for_the_spill(eager):
    from svision_amd.ingest_gpu import LazySeq
    packed = np.frombuffer(eager.seq_packed, np.uint8)
    lazy = LazySeq(packed.size)
    assert lazy.size == len(lazy) == lazy.nbytes == packed.size
    with pytest.raises(RuntimeError):
        lazy[0]                                               # no event: the bases are on the device only, said at once
    lazy.event = threading.Event()
    table = _lazy_twin(eager, lazy)
    first = next(i for i in range(len(eager)) if eager.l_seq[i] > 0 and eager.query_sequence(i) is not None)
    t0 = time.time()

    def spill():
        time.sleep(0.2)
        lazy.attach(packed.copy())
        lazy.event.set()
    threading.Thread(target=spill).start()
    assert table.query_sequence(first) == eager.query_sequence(first)      # blocks until the spill is through
    assert time.time() - t0 >= 0.19
    assert np.asarray(lazy).tobytes() == bytes(eager.seq_packed) and lazy[3] == packed[3]
    failed = LazySeq(5)
    failed.event = threading.Event()
    failed.event.set()                                        # a spill that failed sets the event without attaching anything
    with pytest.raises(RuntimeError):
        failed[0]


def test_a_helper_waits_for_the_ready_flag_of_the_slot(eager, tmp_path):
    """load_shared_sample on a meta with ``lazy_seq``: the table's bases are the slot's seq_packed.bin, mapped once seq.ready is there."""
    d = str(tmp_path / "s0")
    os.makedirs(d)
    packed = np.frombuffer(eager.seq_packed, np.uint8)
    arrays = {}
    names_blob = np.frombuffer(("\n".join(eager.names) + "\n").encode(), np.uint8)
    gap_dtype = __import__("svision_amd.kernels", fromlist=["GAP_DTYPE"]).GAP_DTYPE
    for name, arr in (("tid", eager.tid), ("pos", eager.pos), ("flag", eager.flag), ("mapq", eager.mapq), ("l_seq", eager.l_seq),
                      ("name_id", eager.name_id), ("cig_off", eager.cig_off), ("cigar", eager.cigar), ("names", names_blob),
                      ("seq_off", np.asarray(eager.seq_off, np.int64)), ("gaps", np.empty(0, gap_dtype)),
                      ("gap_off", np.zeros(len(eager) + 1, np.int64)), ("stats", np.zeros((len(eager), 4), np.int32))):
        arr = np.ascontiguousarray(arr)
        arrays[name] = (arr.dtype.str, int(arr.size))
        if arr.size:
            arr.tofile(os.path.join(d, name + ".bin"))
    meta = {"dir": d, "arrays": arrays, "references": eager.references, "lengths": eager.lengths, "min_sv": 50, "n": len(eager), "with_seq": True,
            "header_text": "", "stats_shape": [len(eager), 4], "lazy_seq": int(packed.size)}
    table = ingest.load_shared_sample(meta, None).table
    lazy = table.seq_packed
    assert type(lazy).__name__ == "LazySeq" and lazy._arr is None and lazy.size == packed.size
    t0 = time.time()

    def spill():                                              # the owner's spill thread: the file first, the flag behind it
        time.sleep(0.2)
        packed.tofile(os.path.join(d, "seq_packed.bin"))
        open(os.path.join(d, "seq.ready"), "w").close()
    threading.Thread(target=spill).start()
    rows = [i for i in range(len(eager)) if eager.l_seq[i] > 0][:25]
    assert [table.query_sequence(i) for i in rows] == [eager.query_sequence(i) for i in rows]
    assert time.time() - t0 >= 0.19
    assert np.asarray(lazy).tobytes() == bytes(eager.seq_packed)


def test_subset_and_query_sequence_on_the_lazy_form_equal_the_eager_form(eager):
    from svision_amd.ingest_gpu import LazySeq
    lazy = LazySeq(len(eager.seq_packed))
    lazy.attach(np.frombuffer(eager.seq_packed, np.uint8))
    table = _lazy_twin(eager, lazy)
    assert [table.query_sequence(i) for i in range(len(table))] == [eager.query_sequence(i) for i in range(len(eager))]
    rows = np.arange(1, len(eager), 3)
    a, b = table.subset(rows), eager.subset(rows)
    assert a.seq_packed is lazy and np.array_equal(a.seq_off, b.seq_off)
    assert [a.query_sequence(j) for j in range(len(a))] == [b.query_sequence(j) for j in range(len(b))]
    assert any(s is not None for s in (a.query_sequence(j) for j in range(len(a))))
    assert lazy[2:9].tobytes() == eager.seq_packed[2:9]


def test_the_pack_layout_without_bases_is_what_it_was():
    """The seq_off section sits behind the existing ones: a run without bases reads back the same buffer as before."""
    from svision_amd.ingest_gpu import _pack_layout
    plain, size = _pack_layout(1000, 12345)
    with_seq, size_seq = _pack_layout(1000, 12345, True)
    assert len(plain) == 9 and len(with_seq) == 10 and np.array_equal(with_seq[:9], plain)
    assert int(with_seq[9] - with_seq[8]) >= 8 * 1001 and int(with_seq[8]) % 16 == 0 and size_seq >= int(with_seq[9]) + 16 and size_seq >= size
