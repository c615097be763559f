"""The oracle of the device record sort (svision_amd/csrc/svx_recsort.hip, svision_amd/ingest_sort.py) and the inputs its tests share.

Everything here is NumPy: ``np.argsort(key, kind="stable")`` and fancy indexing.  No product code computes an expected value --
the product's BAM reader and writer only move records between files and tables (tests/test_record_sort_cpu.py pins that they
keep file order)."""
import numpy as np

from svision_amd.io import bam


# ---- the order ----
def key(tid, pos, n_ref):
    """((tid < 0 ? n_ref : tid) << 32) | (uint32)(pos + 1), uint64."""
    tid, pos = np.asarray(tid).astype(np.int64), np.asarray(pos).astype(np.int64)
    hi = np.where(tid < 0, np.int64(n_ref), tid).astype(np.uint64)
    return (hi << np.uint64(32)) | (pos + 1).astype(np.uint64)


def order(tid, pos, n_ref):
    """Input index of the record of every sorted rank: ascending key, ties in input order."""
    return np.argsort(key(tid, pos, n_ref), kind="stable")


def gather_segments(data, off, rows):
    """CSR (data, off [n + 1]) with its segments laid out in the order ``rows`` -> (data_out, off_out)."""
    off = np.asarray(off, np.int64)
    rows = np.asarray(rows, np.int64)
    lens = off[rows + 1] - off[rows]
    out_off = np.zeros(rows.size + 1, np.int64)
    out_off[1:] = np.cumsum(lens)
    idx = np.repeat(off[rows] - out_off[:-1], lens) + np.arange(int(out_off[-1]), dtype=np.int64)
    return np.asarray(data)[idx], out_off


# ---- tables ----
def reorder_table(table, rows, header_text=None):
    """The table of a file that holds ``table``'s records in the order ``rows``, as a decoder returns it: every array fancy-indexed,
    QNAME ids re-assigned by first occurrence in the new order, the bases dense in the new order."""
    rows = np.asarray(rows, np.int64)
    cigar, cig_off = gather_segments(table.cigar, table.cig_off, rows)
    old = table.name_id[rows]
    _u, first = np.unique(old, return_index=True)
    first_sorted = np.sort(first)                               # positions where a name occurs for the first time, ascending
    new_of_old = np.full(len(table.names), -1, np.int64)
    new_of_old[old[first_sorted]] = np.arange(first_sorted.size)
    names = [table.names[int(i)] for i in old[first_sorted]]
    seq_packed = seq_off = None
    if table.seq_packed is not None:
        n_bytes = (table.l_seq.astype(np.int64) + 1) // 2
        src_off = np.append(np.asarray(table.seq_off, np.int64), 0)
        packed = np.frombuffer(bytes(table.seq_packed), np.uint8)
        pieces = [packed[int(src_off[r]):int(src_off[r]) + int(n_bytes[r])] for r in rows]
        seq_packed = np.concatenate(pieces).tobytes() if pieces else b""
        seq_off = np.zeros(rows.size, np.int64)
        seq_off[1:] = np.cumsum(n_bytes[rows])[:-1]
    return bam.AlignmentTable(table.references, table.lengths, table.tid[rows], table.pos[rows], table.flag[rows], table.mapq[rows],
                              table.l_seq[rows], new_of_old[old].astype(np.int32), names, cigar, cig_off,
                              table.header_text if header_text is None else header_text, seq_packed, seq_off)


def assert_same_table(got, want, with_seq=False, what=""):
    """Array for array: fields, CIGARs, QNAME ids and the name list, and (``with_seq``) every record's bases."""
    for f in ("tid", "pos", "flag", "mapq", "l_seq", "name_id", "cig_off"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), (what, f)
    assert np.array_equal(np.asarray(got.cigar), np.asarray(want.cigar)), (what, "cigar")
    assert list(got.names) == list(want.names), (what, "names")
    assert list(got.references) == list(want.references) and list(got.lengths) == list(want.lengths), (what, "references")
    if with_seq:
        assert got.seq_packed is not None and want.seq_packed is not None, (what, "seq")
        assert np.array_equal(np.asarray(got.seq_off, np.int64), np.asarray(want.seq_off, np.int64)), (what, "seq_off")
        assert bytes(got.seq_packed) == bytes(want.seq_packed), (what, "seq_packed")
        for i in (0, len(want) // 2, len(want) - 1):
            assert got.query_sequence(i) == want.query_sequence(i), (what, "bases", i)


def retitled(text, sort_order):
    """A header text whose @HD line says ``SO:<sort_order>``; ``None``: no @HD line at all."""
    lines = [l for l in text.split("\n") if l and not l.startswith("@HD")]
    head = [] if sort_order is None else ["@HD\tVN:1.6\tSO:%s" % sort_order]
    return "\n".join(head + lines) + "\n"


def shuffled_files(golden_bam, out_dir, seed, sort_order="unsorted"):
    """The records of a golden (sorted) BAM in a seeded random order, written with the product's writer under an @HD line that says
    so -> (path of the shuffled file, path of the file sorted stably from it (SO:coordinate, with its .bai), the table the sorted
    file must decode to).  Both files carry the read bases."""
    import os
    src = bam.read_bam(golden_bam, with_seq=True)
    perm = np.random.default_rng(seed).permutation(len(src))
    name = os.path.splitext(os.path.basename(golden_bam))[0]
    shuffled = reorder_table(src, perm, retitled(src.header_text, sort_order))
    path = os.path.join(str(out_dir), name + ".shuffled.bam")
    bam.write_bam(path, shuffled, with_seq=True, index=False)
    want = reorder_table(shuffled, order(shuffled.tid, shuffled.pos, len(src.references)), retitled(src.header_text, "coordinate"))
    sorted_path = os.path.join(str(out_dir), name + ".sorted.bam")
    bam.write_bam(sorted_path, want, with_seq=True, index=True)
    return path, sorted_path, want


# ---- crafted keys for the kernel tests ----
def key_cases(tile):
    """[(name, tid int32, pos int32, n_ref, pos_bits)]: the sizes around the wave and the tile with random keys, and the key
    patterns at 3 tiles + 1."""
    rng = np.random.default_rng(20)
    out = []

    def random_keys(n, n_ref, pos_bits, unmapped=0.1):
        tid = rng.integers(0, n_ref, n).astype(np.int32)
        tid[rng.random(n) < unmapped] = -1
        top = min((1 << pos_bits) - 2, (1 << 31) - 2)
        pos = rng.integers(-1, top, n, endpoint=True).astype(np.int32)
        return tid, pos

    for n in (0, 1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 1):
        out.append(("random/n%d" % n,) + random_keys(n, 2, 25) + (2, 25))
    n = 3 * tile + 1
    for n_ref in (1, 2, 3366):
        for pos_bits in (8, 25, 32):
            out.append(("random/ref%d/bits%d" % (n_ref, pos_bits),) + random_keys(n, n_ref, pos_bits) + (n_ref, pos_bits))
    out.append(("all_equal", np.full(n, 1, np.int32), np.full(n, 77, np.int32), 2, 25))
    alt = np.arange(n) % 2
    out.append(("alternating", np.where(alt, 0, 1).astype(np.int32), np.where(alt, 9, 300_000).astype(np.int32), 2, 25))
    tid, pos = random_keys(n, 3366, 32)
    o = order(tid, pos, 3366)
    out.append(("sorted", tid[o], pos[o], 3366, 32))
    out.append(("reversed", tid[o][::-1].copy(), pos[o][::-1].copy(), 3366, 32))
    # 32 + 12 key bits, six digits: the top one holds tid's bits 8 and up, the lowest pos + 1's bits 0..7
    out.append(("top_digit_only", (rng.integers(0, 14, n) * 256).astype(np.int32), np.full(n, 1000, np.int32), 3366, 32))
    low = rng.integers(-1, 254, n, endpoint=True).astype(np.int32)
    low[:4] = (-1, 254, 254, -1)                                # digit values 0 and 255
    out.append(("low_digit_only", np.zeros(n, np.int32), low, 3366, 32))
    tid, pos = random_keys(n, 2, 32, unmapped=0.0)
    pos[::7] = (1 << 31) - 2                                    # the largest position a BAM can name
    tid[3::5] = -1                                              # records without a reference, scattered through the input
    pos[3::5] = -1
    out.append(("max_pos_and_unmapped", tid, pos, 2, 32))
    for big in (300_001, 2_200_003):                            # 147 and 1,075 tiles: several chunks of the table's scan, then several steps of its top level
        out.append(("random/n%d" % big,) + random_keys(big, 3366, 28) + (3366, 28))
    return out


def segment_lengths(seed=3, tail=40):
    """Lengths of the segmented-gather test: runs of empty segments at both ends, the lengths around a dword and a wave, one
    segment of 70,000 elements, random ones between."""
    rng = np.random.default_rng(seed)
    return np.asarray([0] * 5 + [0, 1, 2, 3, 4, 5, 63, 64, 65, 70_000] + rng.integers(0, 300, tail).tolist() + [7, 0, 0, 0, 0], np.int64)
