"""svision_amd.io.bai.bai_bytes (vectorised NumPy) == tests/htslike.write_bai (a record-by-record reading of htslib's indexer),
byte for byte, on the record lists of the index-build cases -- walked out of the files by tests/baicases.walk (zlib + struct)."""
import numpy as np
import pytest

from svision_amd.io import bai, bam
from tests import baicases, htslike


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, walk) of the cases: flushed blocks (levels 1 and 9), straddling blocks, a CG-tag record, records longer than
    a block, the decoy."""
    d = tmp_path_factory.mktemp("bai_cpu")
    out = {}
    for name, recs, level, policy in (("flushed1", baicases.short_records(), 1, "htslib"), ("flushed9", baicases.short_records(seed=3), 9, "htslib"),
                                      ("straddling", baicases.short_records(seed=4), 1, "stream"), ("cg", baicases.short_records(seed=6, n=120, cg=True), 6, "htslib")):
        path = str(d / (name + ".bam"))
        htslike.write_bam(path, baicases.REFS, recs, level=level, policy=policy)
        out[name] = (path, baicases.walk(path))
    out["long"] = (str(d / "long.bam"), baicases.write_long(str(d / "long.bam"))[0])
    out["decoy"] = (str(d / "decoy.bam"), baicases.write_decoy(str(d / "decoy.bam"))[0])
    return out


@pytest.mark.parametrize("name", ["flushed1", "flushed9", "straddling", "cg", "long", "decoy"])
def test_bai_bytes_equals_htslike(files, name, tmp_path):
    path, walked = files[name]
    want = baicases.expected_bai(tmp_path, walked)
    got = bai.bai_bytes(*baicases.arrays(walked))
    assert got == want
    if name in ("flushed1", "flushed9", "straddling", "cg"):          # the index htslike wrote next to the file itself, from its own offsets
        assert got == open(path + ".bai", "rb").read()
    index = str(tmp_path / "got.bai")
    with open(index, "wb") as f:
        f.write(got)
    spans, linear = bam.read_bai(index), bam.read_bai_linear(index)
    assert len(spans) == len(linear) == 3 and spans[1] is None and linear[1] is None
    for t in (0, 2):
        first = next(i for i, r in enumerate(walked.records) if r["tid"] == t)
        last = max(i for i, r in enumerate(walked.records) if r["tid"] == t)
        assert spans[t] == (walked.voffs[first], walked.voffs[last + 1]) == linear[t][:2]
        assert linear[t][2].size == max((r["pos"] + (htslike.ref_len(r["cigar"]) or 1) - 1 >> 14) + 1 for r in walked.records if r["tid"] == t)
        assert (np.diff(linear[t][2].astype(np.int64)) >= 0).all() and int(linear[t][2][0]) == walked.voffs[first]


def test_the_walk_sees_what_the_cases_are_about(files):
    """The cases hold what they are named for (so that no comparison passes by missing its target)."""
    cg = [r for r in files["cg"][1].records if len(r["cigar"]) > 65535]
    assert len(cg) == 1 and htslike.ref_len(cg[0]["cigar"]) == 33_540
    for name in ("flushed1", "flushed9"):
        w = files[name][1]
        assert all(v & 0xFFFF == 0 or w.block_of(o) == w.block_of(w.offsets[i - 1]) for i, (o, v) in enumerate(zip(w.offsets, w.voffs)) if i)
        assert sum(r["tid"] < 0 for r in w.records) == 9 and any(r["flag"] & 4 and r["tid"] >= 0 for r in w.records)
    w = files["straddling"][1]
    inner = [f for f in w.first[1:-1] if f != baicases.NO_START]
    assert len(inner) >= 10 and all(f % baicases.BLOCK for f in inner)


def test_offsets_behind_a_blocks_last_byte():
    """coffset << 16 | offset in the block; exactly behind a block's last byte = offset 0 of the next block that holds data, of the
    file's last block where none does."""
    dst = np.asarray([0, 100, 100, 250, 250], np.uint64)        # block 1 and block 3 (the last) hold no byte
    coff = np.asarray([0, 60, 88, 170], np.uint64)
    got = bai.virtual_offsets(dst, coff, np.asarray([0, 99, 100, 249, 250], np.uint64))
    assert got.tolist() == [0, 99, 88 << 16, 88 << 16 | 149, 170 << 16]


def test_unsorted_records_are_refused(files):
    n_ref, tid, pos, end, flag, voff, voff_end = baicases.arrays(files["straddling"][1])
    for i, j in ((10, 11), (0, len(tid) - 1)):                  # two neighbours swapped; a record without a reference in front of all others
        order = np.arange(len(tid))
        order[[i, j]] = order[[j, i]]
        assert (tid[i], pos[i]) != (tid[j], pos[j])
        with pytest.raises(ValueError, match="not coordinate-sorted"):
            bai.bai_bytes(n_ref, tid[order], pos[order], end[order], flag[order], voff, voff_end)
    with pytest.raises(ValueError):
        bai.bai_bytes(2, tid, pos, end, flag, voff, voff_end)   # a record of reference 2 in a dictionary of two
    assert bai.bai_bytes(3, [], [], [], [], [], []) == b"BAI\x01" + (3).to_bytes(4, "little") + bytes(8 * 3) + bytes(8)
