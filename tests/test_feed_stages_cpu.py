"""The chromosome feed's pure pieces (svision_amd/ingest.py) without a GPU: which references the host reader takes after the
device engine refused a pass, how the slice margin grows, and a host-decoded table's way through a shared-memory slot to
what a helper process maps (put_table / part_meta / load_shared_sample over one list of file names)."""
import os
import types

import numpy as np
import pytest

from svision_amd import ingest
from svision_amd.io import bam
from svision_amd.sample import Sample
from tests import helpers


def _units(*tids):
    return [types.SimpleNamespace(tid=t) for t in tids]


def test_the_host_takes_the_references_a_refusal_names():
    rest = _units(3, 3, 4, 5, 5, 7)                               # slices of four references, in file order
    # named references: everything up to the LAST unit of a named one (the device engine goes on behind them), each once
    assert ingest.host_takes(rest, [4], 1) == [3, 4]
    assert ingest.host_takes(rest, [3], 1) == [3]
    assert ingest.host_takes(rest, [5, 3], 2) == [3, 4, 5]
    # nothing named -- or only references that are not waiting any more: the one the consumer waits for is blamed
    assert ingest.host_takes(rest, None, 1) == [3]
    assert ingest.host_takes(rest, [], 2) == [3]
    assert ingest.host_takes(rest, [1], 1) == [3]
    # the third refusal: the host reader takes the rest of the file, whatever is named
    assert ingest.host_takes(rest, [4], 3) == [3, 4, 5, 7]
    assert ingest.host_takes(rest, None, 3) == [3, 4, 5, 7]
    assert ingest.host_takes(rest, [3], 4) == [3, 4, 5, 7]
    # a refusal behind the last unit leaves nothing to take
    assert ingest.host_takes([], [4], 1) == [] and ingest.host_takes([], None, 3) == []


def test_the_margin_grows_to_twice_what_was_needed_in_index_bins():
    assert ingest.grow_margin(10_000, 16_384) == 32_768           # at least twice the old margin
    assert ingest.grow_margin(100_000, 16_384) == 212_992         # twice the need, rounded up to 16 kb
    assert ingest.grow_margin(8_192, 1) == 16_384 and ingest.grow_margin(0, 0) == 0
    for needed, margin in ((1, 1), (70_001, 65_536), (1_234_567, 16_384)):
        got = ingest.grow_margin(needed, margin)
        assert got % 16_384 == 0 and 0 <= got - max(2 * needed, 2 * margin) < 16_384


def test_the_slot_array_names_are_the_files_of_a_part():
    names = [n for n, _d in ingest.TABLE_ARRAYS + ingest.SEQ_ARRAYS] + list(ingest.SCAN_ARRAYS)
    assert names == "tid pos flag mapq l_seq name_id cig_off cigar names seq_off seq_packed gaps gap_off stats".split()


@pytest.mark.parametrize("with_seq", [False, True])
def test_a_host_decoded_table_comes_back_from_its_slot(tmp_path, with_seq):
    """What ChromosomeFeed._host_parts and _hand_over do with a table of the host engine, and what a helper reads of it."""
    path = os.path.join(helpers.GOLDEN, "hash_collect.bam" if with_seq else "collect_small.bam")
    stream = bam.BamStream(path, with_seq=with_seq, threads=2)
    tables = list(stream)
    stream.close()
    assert tables and sum(len(t) for t in tables) == len(bam.read_bam(path))
    pool = ingest._SlotPool(str(tmp_path))
    for table in tables:
        slot = pool.take()
        ingest.put_table(slot, table, with_seq)
        sample = Sample.with_scan(table, None, 50, helpers.oracle_scan(table, 50))
        meta = ingest.part_meta(slot, table, sample, table.references, table.lengths, 50, with_seq)
        want = [n for n, _d in ingest.TABLE_ARRAYS + (ingest.SEQ_ARRAYS if with_seq else ())] + list(ingest.SCAN_ARRAYS)
        assert list(meta["arrays"]) == want and meta["dir"] == slot.dir and meta["n"] == len(table) > 0
        assert sorted(os.listdir(slot.dir)) == sorted(n + ".bin" for n in want if meta["arrays"][n][1])
        assert set(meta) == {"dir", "arrays", "references", "lengths", "min_sv", "n", "with_seq", "header_text", "stats_shape"}
        back = ingest.load_shared_sample(meta, None)
        t = back.table
        for name in ("tid", "pos", "flag", "mapq", "l_seq", "name_id", "cig_off", "cigar"):
            got, exp = getattr(t, name), getattr(table, name)
            assert got.dtype == exp.dtype and np.array_equal(got, exp), name
        assert t.names == table.names and t.references == table.references and t.header_text == table.header_text
        if with_seq:
            assert np.array_equal(t.seq_off, table.seq_off) and bytes(t.seq_packed) == bytes(table.seq_packed)
            rows = [i for i in range(len(table)) if table.l_seq[i] > 0][:20]
            assert rows and [t.query_sequence(i) for i in rows] == [table.query_sequence(i) for i in rows]
        else:
            assert t.seq_packed is None and t.seq_off is None
        assert back.gaps.tobytes() == sample.gaps.tobytes() and np.array_equal(back.gap_off, sample.gap_off)
        assert np.array_equal(back.stats, sample.stats) and back.stats.shape == sample.stats.shape
        pool.give(slot.dir)
