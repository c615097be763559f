"""sort_bam with a memory budget below the file's records (svision_amd/sort.py: the output's record stream filled in spans, a pass over
the input for each): the unsorted files of tests/test_gpu_sort_write.py and a sorted file retitled ``unsorted``, each with a budget
of a fifth of its record bytes.  The output and its .bai are the in-core run's byte for byte -- whose contents that test checks --,
the record buffer stays within the budget + two records, a record straddles a span's edge, and the ranges read again are the ones
the test counts itself from the pass's ``range_records`` and the NumPy order.  Budgets of one byte and of all the records, a BAM
without records, broken inputs and the command line's ``--memory`` / ``SVX_SORT_MEMORY``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from svision_amd.io import bam
from tests import baicases, helpers, htslike, sortcases
from tests.test_gpu_sort_write import _htslike_files

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = htslike.BLOCK
NAMES = ["collect_small", "ont_small", "aligner", "collect_sorted"]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _order_and_offsets(w):
    """The walked input -> (sortcases.order of its records, the offsets of the sorted records in the output's record stream, the
    longest record)."""
    o = sortcases.order(np.asarray([r["tid"] for r in w.records]), np.asarray([r["pos"] for r in w.records]), len(w.references))
    lens = np.diff(np.asarray(list(w.offsets) + [len(w.stream)], np.int64))
    off = np.zeros(o.size + 1, np.int64)
    off[1:] = np.cumsum(lens[o])
    return o, off, int(lens.max())


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> dict: the unsorted path, the input walked, the budget, and sort_bam's outputs in one piece ("core") and in spans
    ("spans") as (path, stats), tables="fixed"; for collect_small also "core_dyn" / "spans_dyn".  Computed once."""
    from svision_amd import sort
    d = str(tmp_path_factory.mktemp("sort_spans"))
    out = {}
    # (seeds with which every range of the pass owns a record of every span, the short last one too: the count of re-read ranges is
    # then ranges x spans)
    for name, seed in (("collect_small", 12), ("ont_small", 12)):
        path, _sorted, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, name + ".bam"), d, seed)
        out[name] = dict(path=path)
    out["aligner"] = dict(path=_htslike_files(d)[0])
    src = bam.read_bam(os.path.join(helpers.GOLDEN, "collect_small.bam"), with_seq=True)
    path = os.path.join(d, "collect_sorted.bam")
    bam.write_bam(path, sortcases.reorder_table(src, np.arange(len(src)), sortcases.retitled(src.header_text, "unsorted")), with_seq=True, index=False)
    out["collect_sorted"] = dict(path=path)
    for name, f in out.items():
        assert bam.read_bam_header(f["path"]).sort_order != "coordinate"
        f["walked"] = w = baicases.walk(f["path"])
        f["record_bytes"] = len(w.stream) - w.header_end
        f["memory_bytes"] = max(f["record_bytes"] // 5 // BLOCK, 1) * BLOCK
        f["range_bytes"] = max(os.path.getsize(f["path"]) // 6, 1 << 16)
        runs = [("core", None, "fixed"), ("spans", f["memory_bytes"], "fixed")]
        if name == "collect_small":
            runs += [("core_dyn", None, "dynamic"), ("spans_dyn", f["memory_bytes"], "dynamic")]
        for what, memory, tables in runs:
            stats = {}
            p = os.path.join(d, "%s.%s.bam" % (name, what))
            assert sort.sort_bam(f["path"], p, device=DEV, stats=stats, range_bytes=f["range_bytes"], memory_bytes=memory, tables=tables) == p
            f[what] = (p, stats)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_spans_write_the_in_core_files(files, name):
    from svision_amd import sort
    f = files[name]
    (core, core_stats), (out, stats) = f["core"], f["spans"]
    assert _read(out) == _read(core) and _read(out + ".bai") == _read(core + ".bai")
    assert _read(out).endswith(htslike.EOF_BLOCK) and stats["records"] == len(f["walked"].records) > 0
    if name == "collect_small":
        assert _read(f["spans_dyn"][0]) == _read(f["core_dyn"][0]) and _read(f["spans_dyn"][0] + ".bai") == _read(f["core_dyn"][0] + ".bai")
        assert f["spans_dyn"][1]["dynamic_blocks"] > 0 and f["spans_dyn"][1]["spans"] == stats["spans"] and _read(f["core_dyn"][0]) != _read(core)
    print(name, {k: stats[k] for k in ("ranges", "spans", "span_range_reads", "range_records", "stream_bytes", "chunks")}, core_stats["stream_bytes"])
    assert stats["spans"] >= 3 and stats["ranges"] >= 4 and set(stats["seconds"]) == set(sort.STAGES), stats
    assert core_stats["spans"] == 1 and core_stats["span_range_reads"] == 0 and core_stats["ranges"] == stats["ranges"]
    assert core_stats["range_records"] == stats["range_records"] and sum(stats["range_records"]) == stats["records"]
    # the record buffer: within the budget + two records, and below the whole stream's
    order, off, longest = _order_and_offsets(f["walked"])
    assert stats["stream_bytes"] <= f["memory_bytes"] + 2 * longest + 4
    assert stats["stream_bytes"] < core_stats["stream_bytes"] == f["record_bytes"] + 4
    # the spans, from the walked file alone: a record straddles an edge
    span = f["memory_bytes"]
    edges = np.arange(span, f["record_bytes"], span)
    assert stats["spans"] == edges.size + 1
    assert (off[np.searchsorted(off, edges, "right") - 1] != edges).any()
    # the ranges read again: per span the ranges that own a record which touches it
    owner = np.repeat(np.arange(stats["ranges"]), stats["range_records"])
    reads = 0
    for lo in range(0, f["record_bytes"], span):
        hi = min(lo + span, f["record_bytes"])
        touching = np.flatnonzero((off[:-1] < hi) & (off[1:] > lo))
        reads += np.unique(owner[order[touching]]).size
    assert stats["span_range_reads"] == reads
    if name in ("collect_small", "ont_small"):
        assert reads == stats["ranges"] * stats["spans"]
    if name == "collect_sorted":
        assert reads <= stats["ranges"] + stats["spans"]
    assert not [n for n in os.listdir(os.path.dirname(out)) if n.endswith(".tmp")]


def test_other_budgets(files, tmp_path):
    from svision_amd import sort
    f = files["aligner"]
    core = _read(f["core"][0]), _read(f["core"][0] + ".bai")
    # one byte: a block a span
    stats = {}
    p = sort.sort_bam(f["path"], str(tmp_path / "one.bam"), device=DEV, stats=stats, memory_bytes=1)
    assert (_read(p), _read(p + ".bai")) == core
    assert stats["spans"] == -(-f["record_bytes"] // BLOCK) == stats["chunks"] and stats["ranges"] == 1 and stats["span_range_reads"] == stats["spans"]
    # the records fit: today's path
    for memory in (f["record_bytes"], f["record_bytes"] + 1, 1 << 40):
        stats = {}
        p = sort.sort_bam(f["path"], str(tmp_path / "fits.bam"), device=DEV, stats=stats, range_bytes=f["range_bytes"], memory_bytes=memory)
        assert (_read(p), _read(p + ".bai")) == core and stats["spans"] == 1 and stats["span_range_reads"] == 0
        assert stats["stream_bytes"] == f["record_bytes"] + 4
    # a byte short: two spans
    stats = {}
    p = sort.sort_bam(f["path"], str(tmp_path / "short.bam"), device=DEV, stats=stats, memory_bytes=f["record_bytes"] - 1, chunk_bytes=3 * BLOCK)
    assert (_read(p), _read(p + ".bai")) == core and stats["spans"] == 2
    assert not [n for n in os.listdir(str(tmp_path)) if n.endswith(".tmp")]


def test_header_only(tmp_path):
    from svision_amd import sort
    path = str(tmp_path / "empty.bam")
    htslike.write_bam(path, baicases.REFS, [], level=1, policy="stream", index=False)
    a = sort.sort_bam(path, str(tmp_path / "a.bam"), device=DEV)
    stats = {}
    b = sort.sort_bam(path, str(tmp_path / "b.bam"), device=DEV, memory_bytes=1, stats=stats)
    assert _read(a) == _read(b) and _read(a + ".bai") == _read(b + ".bai") and _read(b).endswith(htslike.EOF_BLOCK)
    assert stats["records"] == 0 and stats["spans"] == 1 and stats["span_range_reads"] == 0


def test_broken_inputs_leave_nothing(files, tmp_path):
    from svision_amd import sort
    raw = _read(files["collect_small"]["path"])
    cut = str(tmp_path / "cut.bam")
    with open(cut, "wb") as f:
        f.write(raw[:len(raw) * 2 // 3])
    flipped = bytearray(raw)
    blocks = baicases.bgzf_blocks(raw)
    flipped[blocks[len(blocks) // 2][0] + 18 + 40] ^= 0x55          # inside the DEFLATE payload of a block in the middle of the file
    flip = str(tmp_path / "flipped.bam")
    with open(flip, "wb") as f:
        f.write(bytes(flipped))
    before = sorted(os.listdir(str(tmp_path)))
    for bad in (cut, flip):
        with pytest.raises(sort.SortWriteError):
            sort.sort_bam(bad, str(tmp_path / "never.bam"), device=DEV, range_bytes=1 << 16, chunk_bytes=1 << 16, memory_bytes=4 * BLOCK)
        assert sorted(os.listdir(str(tmp_path))) == before


def test_command_line_memory(files, tmp_path):
    """One child process with --memory 128K, one with SVX_SORT_MEMORY=131072 and no option: the in-core file, written in spans;
    --memory nonsense is refused."""
    f = files["collect_small"]
    base = {k: v for k, v in os.environ.items() if k not in ("SVX_SORT_MEMORY", "SVX_SORT_TABLES")}
    want = _read(f["core"][0]), _read(f["core"][0] + ".bai")
    for what, args, env in (("option", ["--memory", "128K"], {}), ("variable", [], {"SVX_SORT_MEMORY": "131072"})):
        out, js = str(tmp_path / (what + ".bam")), str(tmp_path / (what + ".json"))
        r = subprocess.run([sys.executable, "-m", "svision_amd.sort", f["path"], "-o", out, "--device", DEV, "--stats-json", js] + args,
                           capture_output=True, text=True, timeout=600, env=dict(base, PYTHONPATH=ROOT, **env))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert (_read(out), _read(out + ".bai")) == want
        with open(js) as fh:
            stats = json.load(fh)
        assert stats["spans"] == -(-f["record_bytes"] // (2 * BLOCK)) > 1 and stats["memory_bytes"] == 131072 and " span(s)" in r.stdout
    r = subprocess.run([sys.executable, "-m", "svision_amd.sort", f["path"], "-o", str(tmp_path / "no.bam"), "--memory", "nonsense"],
                       capture_output=True, text=True, timeout=600, env=dict(base, PYTHONPATH=ROOT))
    assert r.returncode != 0 and "--memory" in r.stderr and not os.path.exists(str(tmp_path / "no.bam"))
