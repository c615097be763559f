"""The SAM kernels (svision_amd/csrc/svx_sam.hip: svx_sam_lines, svx_sam_measure, svx_sam_encode) on the cases of tests/sam_cases.py, the
text cut into chunks of 4 KB, 64 KB and one piece: the records are tests/htslike.py's byte for byte, nothing is written outside them,
a second launch gives the same bytes, and the lines the kernels hand to the host are exactly the six the case list names."""
import numpy as np
import pytest
import torch

from svision_amd import kernels
from svision_amd.io import sam
from tests import htslike, sam_cases, samtext

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xA5
GUARD = 256


@pytest.fixture(scope="module")
def case():
    """The cases' lines, htslike's record of each, and the reference table on the device: computed once."""
    recs = sam_cases.records()
    lines = [samtext.line(r, sam_cases.REFS) for r in recs]
    want = [htslike.encode_record(samtext.for_htslike(r)) for r in recs]
    return dict(recs=recs, lines=lines, want=want, table=kernels.sam_ref_table([r[0] for r in sam_cases.REFS], DEV))


def _upload(data):
    """A chunk on the device with the kernels' slack behind it, the slack filled with bytes that are no text."""
    d = torch.full((len(data) + kernels.SAM_SLACK,), SENTINEL, dtype=torch.uint8, device=DEV)
    if data:
        d[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return d


def _chunks(lines, chunk_bytes, last_newline=True):
    """The lines in chunks of at most chunk_bytes, cut behind newlines, a longer line alone -> [(first line, number of lines, bytes)]."""
    out, first, cur = [], 0, []
    for i, l in enumerate(lines):
        if cur and sum(len(c) + 1 for c in cur) + len(l) + 1 > chunk_bytes:
            out.append((first, len(cur), b"".join(c + b"\n" for c in cur)))
            first, cur = i, []
        cur.append(l)
    tail = b"".join(c + b"\n" for c in cur)
    out.append((first, len(cur), tail if last_newline else tail[:-1]))
    return out


@pytest.mark.parametrize("chunk_bytes", [4096, 65536, None], ids=["4K", "64K", "whole"])
def test_records_equal_htslike(case, chunk_bytes):
    lines, want = case["lines"], case["want"]
    refused = set(sam_cases.refused_lines())
    seen_refused = set()
    chunks = _chunks(lines, chunk_bytes or 1 << 40, last_newline=chunk_bytes != 65536)
    assert (len(chunks) > 10) if chunk_bytes == 4096 else (len(chunks) > 3) if chunk_bytes else len(chunks) == 1
    for first, n, data in chunks:
        d_text = _upload(data)
        line_off, n_lines = kernels.sam_lines(d_text, len(data), data.count(b"\n") + 2)
        assert n_lines == n
        starts = np.concatenate([[0], np.cumsum([len(l) + 1 for l in lines[first:first + n]])])
        starts[-1] = len(data)
        assert np.array_equal(line_off[:n + 1].cpu().numpy(), starts)
        d_len, d_tid, d_pos, d_flag, d_span = kernels.sam_measure(d_text, len(data), line_off, n, case["table"])
        length, tid, pos, flag, span = (t.cpu().numpy() for t in (d_len, d_tid, d_pos, d_flag, d_span))
        for i in range(n):
            if first + i in refused:
                assert length[i] == kernels.SAM_HOST, (first + i, length[i])
                seen_refused.add(first + i)
                continue
            rec = case["recs"][first + i]
            assert length[i] == len(want[first + i]), (first + i, length[i], len(want[first + i]))
            assert (tid[i], pos[i], flag[i], span[i]) == (rec["tid"], rec["pos"], rec["flag"], htslike.ref_len(rec["cigar"])), first + i
        # the records end to end between two guards, at a base the kernel subtracts: the chunk-local form and the resident one
        sizes = np.maximum(length, 0).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)])
        for out_base, shift in ((0, GUARD), (123_456_789_000, GUARD + 3)):
            d_off = torch.from_numpy(off[:-1] + out_base + shift).to(DEV)
            d_out = torch.full((int(off[-1]) + shift + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
            d_status = torch.zeros(1, dtype=torch.int32, device=DEV)
            kernels.sam_encode(d_text, len(data), line_off, n, case["table"], d_len, d_off, out_base, d_out, d_status)
            got = d_out.cpu().numpy().tobytes()
            assert int(d_status.item()) == 0
            assert got[:shift] == bytes([SENTINEL]) * shift and got[shift + int(off[-1]):] == bytes([SENTINEL]) * GUARD
            for i in range(n):
                if length[i] >= 0:
                    assert got[shift + int(off[i]):shift + int(off[i + 1])] == want[first + i], first + i
            kernels.sam_encode(d_text, len(data), line_off, n, case["table"], d_len, d_off, out_base, d_out, d_status)
            assert d_out.cpu().numpy().tobytes() == got and int(d_status.item()) == 0
    assert seen_refused == refused


def test_error_codes_and_a_wrong_length(case):
    bad = [(text.split(b"\n")[no - 1], code) for _name, text, no, code in sam_cases.errors() if no is not None]
    good = case["lines"][1]
    data = b"".join(l + b"\n" for l, _code in bad) + good + b"\n"
    d_text = _upload(data)
    line_off, n = kernels.sam_lines(d_text, len(data), len(bad) + 3)
    assert n == len(bad) + 1
    d_len = kernels.sam_measure(d_text, len(data), line_off, n, case["table"])[0]
    assert d_len.cpu().tolist() == [code for _l, code in bad] + [len(case["want"][1])]
    # a record that no longer measures the length it is given is not written, and the call says so
    d_wrong = d_len.clone()
    d_wrong[n - 1] += 1
    d_out = torch.full((GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    d_status = torch.zeros(1, dtype=torch.int32, device=DEV)
    kernels.sam_encode(d_text, len(data), line_off, n, case["table"], d_wrong, torch.zeros(n, dtype=torch.int64, device=DEV), 0, d_out, d_status)
    assert int(d_status.item()) == 1 and bool((d_out == SENTINEL).all())


def test_line_table_edges():
    for data in (b"", b"\n", b"a", b"a\n", b"\n\n", b"a\nb", b"x" * 4095 + b"\n" + b"y" * 4096 + b"\n", b"\n" * 10000 + b"z"):
        d_text = _upload(data)
        line_off, n = kernels.sam_lines(d_text, len(data), data.count(b"\n") + 2)
        want = [0] + [i + 1 for i, c in enumerate(data) if c == 10]
        if data and not data.endswith(b"\n"):
            want.append(len(data))
        assert n == len(want) - 1 and line_off[:n + 1].cpu().tolist() == want, data[:20]
    with pytest.raises(Exception):                                  # a table that cannot hold the lines is refused, not overrun
        kernels.sam_lines(_upload(b"a\nb\nc\n"), 6, 2)
