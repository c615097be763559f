"""The SAM pack kernels (svision_amd/csrc/svx_sam.hip: svx_sam_pack_count, svx_sam_pack_extract) on the cases of tests/sam_cases.py
and tests/sam_pack_cases.py, the text cut into chunks of 4 KB, 64 KB and one piece: every array equals the host program's
(tools/hostwave/sam_pack_main.cpp), the native reader's of the same records written as a BAM, and -- for the lines both roads take --
what svx_sam_encode + the BAM walk leave on the device; nothing is written outside a record's own elements."""
import numpy as np
import pytest
import torch

from svision_amd import _lib, index, kernels
from svision_amd.io import bam, sam
from tests import htslike, sam_cases, sam_pack_cases as pc, samtext
from tests.test_gpu_sam_parse import _chunks, _upload

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xA5
GUARD = 64                                                      # elements in front of and behind every output array


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The lines (the placeholder line, the host's, among them), their records for htslike where it can write them, the host program's
    arrays with and without bases, and the reference table on the device: computed once."""
    recs = sam_cases.records() + [rec for _name, rec in pc.shapes()]
    lines = [samtext.line(r, pc.REFS) for r in recs]
    host_line, host_words = pc.placeholder_line()
    at = len(lines) // 2
    lines = lines[:at] + [host_line] + lines[at:] + pc.tag_lines()
    d = tmp_path_factory.mktemp("pack")
    program = pc.build_program(d)
    text = b"\n".join(lines) + b"\n"
    return dict(recs=recs, lines=lines, host_at=at, host_words=host_words, n_bam=len(recs),
                program={w: pc.run_program(program, d, text, w) for w in (False, True)},
                table=kernels.sam_ref_table([r[0] for r in pc.REFS], DEV), dir=d)


def _guarded(n, dtype):
    """A device array of n elements between two guards, all sentinel bytes -> (the whole, the view the kernel is given)."""
    whole = torch.full(((n + 2 * GUARD) * torch.empty(0, dtype=dtype).element_size(),), SENTINEL, dtype=torch.uint8, device=DEV).view(dtype)
    return whole, whole[GUARD:GUARD + n]


def _guards_untouched(whole, n):
    raw = whole.view(torch.uint8).cpu().numpy()
    size = whole.element_size()
    return bool((raw[:GUARD * size] == SENTINEL).all() and (raw[(GUARD + n) * size:] == SENTINEL).all())


def _pack(case, data, n, with_seq, first):
    """A chunk through the two exports -> (status, fields, counts, per line (words, name bytes, SEQ bytes), the typed field arrays).
    The host's line has its counts in the prefix and keeps its sentinels; so do the guards of every array."""
    d_text = _upload(data)
    line_off, n_lines = kernels.sam_lines(d_text, len(data), data.count(b"\n") + 2)
    assert n_lines == n
    d_status, d_fields, d_counts = kernels.sam_pack_count(d_text, len(data), line_off, n, case["table"], with_seq)
    status, fields, counts = d_status.cpu().numpy(), d_fields.cpu().numpy(), d_counts.cpu().numpy()
    sizes = counts.astype(np.int64)
    host = case["host_at"] - first
    if 0 <= host < n:
        assert status[host] == kernels.SAM_HOST
        sizes[:, host] = len(case["host_words"]), len(b"long_cigar\n"), 5 if with_seq else 0
    off = np.zeros((3, n + 1), np.int64)
    np.cumsum(sizes, axis=1, out=off[:, 1:])
    wholes, out = {}, {}
    for key, dtype, count in (("d_tid", torch.int32, n), ("d_pos", torch.int32, n), ("d_l_seq", torch.int32, n), ("d_flag", torch.int16, n),
                              ("d_mapq", torch.uint8, n), ("d_cigar", torch.int32, int(off[0, -1])), ("d_names", torch.uint8, int(off[1, -1])),
                              ("d_seq", torch.uint8, int(off[2, -1]))):
        if key != "d_seq" or with_seq:
            wholes[key], out[key] = _guarded(count, dtype)
            wholes[key] = (wholes[key], count)
    for _again in range(2):                                     # a second launch gives the same bytes
        kernels.sam_pack_extract(d_text, len(data), line_off, n, case["table"], d_status, list(off[:3 if with_seq else 2]), out)
    for key, (whole, count) in wholes.items():
        assert _guards_untouched(whole, count), key
    got = {k: v.cpu().numpy() for k, v in out.items()}
    pieces = []
    for i in range(n):
        words = got["d_cigar"][off[0, i]:off[0, i + 1]].view(np.uint32)
        name = got["d_names"][off[1, i]:off[1, i + 1]].tobytes()
        bases = got["d_seq"][off[2, i]:off[2, i + 1]].tobytes() if with_seq else b""
        if status[i] != 0:                                      # not this kernel's: every element and byte as it was
            assert (words == 0xA5A5A5A5).all() and set(name + bases) <= {SENTINEL} and got["d_tid"][i] == np.int32(-0x5A5A5A5B) \
                and got["d_mapq"][i] == SENTINEL and got["d_flag"][i] == np.int16(-0x5A5B)
        pieces.append((words, name, bases))
    return d_text, line_off, status, fields, counts, pieces, got


def _encoded_walk(case, d_text, n_bytes, line_off, n, both, with_seq):
    """The lines ``both`` (a mask) through svx_sam_encode and the BAM walk on the device (``with_seq``: svx_bam_walk_count_seq /
    _extract_seq) -> the RecordRange of their records."""
    d_len = kernels.sam_measure(d_text, n_bytes, line_off, n, case["table"])[0]
    length = d_len.cpu().numpy().copy()
    both &= length >= 0
    length[~both] = -1
    sizes = np.maximum(length, 0).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    total = int(off[-1])
    d_raw = torch.zeros((max(total, 1) + 15) // 16 * 16 + 16, dtype=torch.uint8, device=DEV)
    d_status = torch.zeros(1, dtype=torch.int32, device=DEV)
    kernels.sam_encode(d_text, n_bytes, line_off, n, case["table"], torch.from_numpy(length).to(DEV), torch.from_numpy(off[:-1].copy()).to(DEV), 0,
                       d_raw, d_status)
    assert int(d_status.item()) == 0
    rng = index.RecordRange()
    rng.starts, rng.d_raw = np.array([0, total], np.uint64), d_raw
    torch_, lib, dev, clock = index.on_device("the test needs the GPU", DEV)
    index._walk_range(lib, torch_, kernels, dev, rng, with_seq, clock)
    return rng


@pytest.mark.parametrize("with_seq", [False, True], ids=["fields", "bases"])
@pytest.mark.parametrize("chunk_bytes", [4096, 65536, None], ids=["4K", "64K", "whole"])
def test_arrays_equal_the_host_program_and_the_walk(case, chunk_bytes, with_seq):
    lines, prog = case["lines"], case["program"][with_seq]
    chunks = _chunks(lines, chunk_bytes or 1 << 40, last_newline=chunk_bytes != 65536)
    assert (len(chunks) > 10) if chunk_bytes == 4096 else (len(chunks) > 3) if chunk_bytes else len(chunks) == 1
    all_status, all_fields, all_counts, all_pieces, typed = [], [], [], [], {k: [] for k in ("d_tid", "d_pos", "d_l_seq", "d_flag", "d_mapq")}
    for first, n, data in chunks:
        d_text, line_off, status, fields, counts, pieces, got = _pack(case, data, n, with_seq, first)
        all_status.append(status), all_fields.append(fields), all_counts.append(counts)
        all_pieces += pieces
        for k in typed:
            typed[k].append(got[k])
        both = status == 0
        rng = _encoded_walk(case, d_text, len(data), line_off, n, both, with_seq)
        assert rng.n_rec == int(both.sum())
        if rng.n_rec:
            for k in typed:
                assert np.array_equal(getattr(rng, k).cpu().numpy(), got[k][both]), (first, k)
            taken = [p for p, b in zip(pieces, both) if b]
            assert np.array_equal(rng.d_cigar[:rng.words].cpu().numpy().view(np.uint32), np.concatenate([p[0] for p in taken]))
            assert rng.d_names[:rng.name_bytes].cpu().numpy().tobytes() == b"".join(p[1] for p in taken)
            assert rng.d_seq is None or rng.d_seq[:rng.seq_bytes].cpu().numpy().tobytes() == b"".join(p[2] for p in taken)
            assert (rng.d_seq is not None) == with_seq
            sizes = np.array([[len(p[0]), len(p[1]), len(p[2])] for p in taken], np.int64).T
            for key, row in (("d_cig_off", 0), ("d_name_off", 1)) + ((("d_seq_off", 2),) if with_seq else ()):
                assert np.array_equal(getattr(rng, key).cpu().numpy(), np.concatenate([[0], np.cumsum(sizes[row])])), key
    status = np.concatenate(all_status)
    taken = status == 0
    assert np.array_equal(status, prog["status"]) and status[case["host_at"]] == kernels.SAM_HOST and int((~taken).sum()) == 1
    assert np.array_equal(np.concatenate(all_fields, axis=1), prog["fields"]) and np.array_equal(np.concatenate(all_counts, axis=1), prog["counts"])
    for k, key in (("d_tid", "tid"), ("d_pos", "pos"), ("d_l_seq", "l_seq"), ("d_flag", "flag"), ("d_mapq", "mapq")):
        assert np.array_equal(np.concatenate(typed[k])[taken], prog[key][taken]), key
    kept = [p for p, t in zip(all_pieces, taken) if t]
    assert np.array_equal(np.concatenate([p[0] for p in kept]), prog["cigar"])
    assert b"".join(p[1] for p in kept) == prog["names"] and b"".join(p[2] for p in kept) == prog["seq"]
    # the 70,000 operations the encoder leaves to the host are taken here, and their words are the host statement's
    i = next(k for k, l in enumerate(lines) if l.startswith(b"cigar_70000\t"))
    assert np.array_equal(all_pieces[i][0], np.array(sam.cigar_words(lines[i].split(b"\t")[5])[0], np.uint32)) and len(all_pieces[i][0]) == 70000


def test_measure_refuses_what_pack_takes(case):
    line = next(l for l in case["lines"] if l.startswith(b"cigar_70000\t"))
    d_text = _upload(line)
    line_off, n = kernels.sam_lines(d_text, len(line), 2)
    assert n == 1 and kernels.sam_measure(d_text, len(line), line_off, 1, case["table"])[0].cpu().tolist() == [kernels.SAM_HOST]
    status, _fields, counts = kernels.sam_pack_count(d_text, len(line), line_off, 1, case["table"], True)
    assert status.cpu().tolist() == [0] and counts.cpu().numpy()[:, 0].tolist() == [70000, len(b"cigar_70000\n"), 0]


@pytest.fixture(scope="module")
def native(case):
    """The records htslike writes as a BAM, read by the native decoder: written and read once."""
    path = str(case["dir"] / "cases.bam")
    htslike.write_bam(path, pc.REFS, [samtext.for_htslike(r) for r in case["recs"]], level=1, index=False)
    return bam.read_bam(path, with_seq=True)


@pytest.mark.parametrize("chunk_bytes", [4096, 65536, None], ids=["4K", "64K", "whole"])
def test_arrays_equal_the_native_reader(case, native, chunk_bytes):
    """The arrays of the lines, chunk by chunk and end to end, are the native reader's of the same records as a BAM."""
    table, n = native, case["n_bam"]
    lines = [l for k, l in enumerate(case["lines"]) if k != case["host_at"]][:n]
    chunks = _chunks(lines, chunk_bytes or 1 << 40)
    assert (len(chunks) > 10) if chunk_bytes == 4096 else (len(chunks) > 3) if chunk_bytes else len(chunks) == 1
    pieces, got = [], {k: [] for k in ("d_tid", "d_pos", "d_l_seq", "d_flag", "d_mapq")}
    saved, case["host_at"] = case["host_at"], -1
    try:
        for first, n_chunk, data in chunks:
            _d_text, _line_off, status, _fields, _counts, chunk_pieces, chunk_got = _pack(case, data, n_chunk, True, first)
            assert not status.any()
            pieces += chunk_pieces
            for k in got:
                got[k].append(chunk_got[k])
    finally:
        case["host_at"] = saved
    got = {k: np.concatenate(v) for k, v in got.items()}
    assert np.array_equal(got["d_tid"], table.tid) and np.array_equal(got["d_pos"], table.pos) and np.array_equal(got["d_l_seq"], table.l_seq)
    assert np.array_equal(got["d_flag"].view(np.uint16), table.flag) and np.array_equal(got["d_mapq"], table.mapq)
    assert np.array_equal(np.concatenate([p[0] for p in pieces]), np.asarray(table.cigar).view(np.uint32))
    assert np.array_equal(np.concatenate([[0], np.cumsum([len(p[0]) for p in pieces])]), table.cig_off)
    assert [p[1][:-1].decode() for p in pieces] == [table.names[int(i)] for i in table.name_id]
    assert b"".join(p[2] for p in pieces) == bytes(table.seq_packed)


def test_more_lines_than_a_launch_has_waves(case):
    """The grid is bounded (4,096 workgroups of 4 waves): 40,000 short lines make every wave take a second and a third line."""
    base = sam_cases.records()[0]
    lines = [samtext.line(dict(base, qname="r%d" % i, pos=i, tid=i % 5, cigar=[(1 + i % 9, "M"), (i % 3 + 1, "I")], seq="ACGTN"[:i % 6] or "*"),
                          pc.REFS) for i in range(40000)]
    data = b"\n".join(lines) + b"\n"
    saved, case["host_at"] = case["host_at"], -1
    try:
        _d_text, _line_off, status, fields, counts, pieces, got = _pack(case, data, len(lines), True, 0)
    finally:
        case["host_at"] = saved
    i = np.arange(40000)
    assert not status.any() and np.array_equal(got["d_pos"], i) and np.array_equal(got["d_tid"], i % 5) and np.array_equal(got["d_l_seq"], i % 6)
    assert np.array_equal(counts[0], np.full(40000, 2)) and np.array_equal(counts[2], (i % 6 + 1) // 2)
    for k in (0, 16383, 16384, 16385, 32768, 39999):
        want = pc.expected(lines[k], True)
        assert (pieces[k][0].tolist(), pieces[k][1], pieces[k][2]) == (want[2], want[3], want[4]), k
    assert b"".join(p[1] for p in pieces) == b"".join(b"r%d\n" % k for k in range(40000))


def test_errors_report_the_right_line(case):
    bad = pc.bad_lines()
    good = case["lines"][3]
    lines = [good] * 5
    for k, (line, _code) in enumerate(bad):
        lines += [line] + [good] * (k % 3)
    data = b"\n".join(lines) + b"\n"
    d_text = _upload(data)
    line_off, n = kernels.sam_lines(d_text, len(data), len(lines) + 2)
    status = kernels.sam_pack_count(d_text, len(data), line_off, n, case["table"], True)[0].cpu().numpy()
    codes = {line: code for line, code in bad}
    assert n == len(lines) and status.tolist() == [codes.get(l, 0) for l in lines]


def test_the_wrapper_refuses_offsets_outside_the_arrays(case):
    line = case["lines"][3] + b"\n"
    d_text = _upload(line)
    line_off, n = kernels.sam_lines(d_text, len(line), 3)
    d_status, _f, d_counts = kernels.sam_pack_count(d_text, len(line), line_off, n, case["table"], False)
    counts = d_counts.cpu().numpy()
    out = {"d_tid": torch.zeros(1, dtype=torch.int32, device=DEV), "d_pos": torch.zeros(1, dtype=torch.int32, device=DEV),
           "d_l_seq": torch.zeros(1, dtype=torch.int32, device=DEV), "d_flag": torch.zeros(1, dtype=torch.int16, device=DEV),
           "d_mapq": torch.zeros(1, dtype=torch.uint8, device=DEV), "d_cigar": torch.zeros(1, dtype=torch.int32, device=DEV),
           "d_names": torch.zeros(int(counts[1, 0]) - 1, dtype=torch.uint8, device=DEV)}
    with pytest.raises(_lib.SvxError):
        kernels.sam_pack_extract(d_text, len(line), line_off, n, case["table"], d_status, [np.array([0, counts[0, 0]]), np.array([0, counts[1, 0]])], out)
