"""sort_bam on a BAM that arrives through a pipe, taken in one pass (svision_amd/sort_sources.py: BamPipeSource over index.stream_ranges, under
``pipe_bam="stream"``): the two files written must be, byte for byte, those of the same bytes read from a regular file -- in core with
no spool file at any moment, beyond the budget through the spool, among several inputs through the copy as it is -- and a failure leaves
nothing and ends the writer.  The cases are those of tests/pipebam_cases.py; in-process tests read a FIFO fed by a daemon thread, the
command line gets the BAM on its standard input."""
import os
import subprocess
import sys

import pytest
import torch  # noqa: F401  (before the first BAM is read: libsvx.so must find the HIP runtime torch brings, not load another)

from tests import htslike, pipebam_cases as pb, samtext

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("hifi", "ont", "stored")


@pytest.fixture(scope="module")
def want(tmp_path_factory):
    """(name, tables) -> (the .bam, the .bai that sort_bam(the file) writes, the records' bytes): sorted once, left unchanged."""
    from svision_amd import sort
    d, out = str(tmp_path_factory.mktemp("pipe_bam_sort")), {}
    for name in CASES + ("none",):
        for tables in ("fixed", "dynamic"):
            p, stats = os.path.join(d, "%s.%s.bam" % (name, tables)), {}
            sort.sort_bam(pb.case(name)["path"], p, device=DEV, tables=tables, stats=stats)
            assert "pipe" not in stats and stats["records"] == pb.case(name)["n"]
            out[name, tables] = (open(p, "rb").read(), open(p + ".bai", "rb").read(), stats["stream_bytes"] - 4)
    return out


def _same_files(want, path):
    assert open(path, "rb").read() == want[0]
    assert open(path + ".bai", "rb").read() == want[1]
    assert sorted(os.listdir(os.path.dirname(path))) == sorted(os.path.basename(path) + e for e in ("", ".bai"))


class _Watch:
    """tempfile.mkstemp of a run, recorded: the name of every file the sort created beside its output (each starts as a temporary)."""

    def __init__(self, monkeypatch):
        import tempfile
        self.names, mkstemp = [], tempfile.mkstemp

        def watched(*a, **kw):
            fd, name = mkstemp(*a, **kw)
            self.names.append(os.path.basename(name))
            return fd, name
        monkeypatch.setattr(tempfile, "mkstemp", watched)


@pytest.mark.parametrize("range_bytes", [64 << 10, None], ids=["64K", "default"])
@pytest.mark.parametrize("tables", ["fixed", "dynamic"])
@pytest.mark.parametrize("name", CASES)
def test_a_bam_pipe_in_core_gives_the_files_of_the_file_road(want, name, tables, range_bytes, tmp_path, monkeypatch):
    from svision_amd import sort
    c, watch = pb.case(name), _Watch(monkeypatch)
    fifo = pb.Fifo(tmp_path, c["data"])
    out, stats = str(tmp_path / "out.bam"), {}
    assert sort.sort_bam(fifo.path, out, device=DEV, tables=tables, range_bytes=range_bytes, stats=stats, pipe_bam="stream") == out
    assert fifo.done() and not fifo.broke
    _same_files(want[name, tables], out)
    pipe, room = stats["pipe"], want[name, tables][2]
    assert pipe["mode"] == "in_core" and pipe["holds"] == "bam" and pipe["spool_bytes"] == 0
    assert pipe["compressed_bytes"] == pipe["text_bytes"] == len(c["data"])
    assert "input" not in stats and "host_lines" not in stats and stats["records"] == c["n"] and stats["spans"] == 1
    assert set(stats["seconds"]) == set(sort.STAGES) and stats["seconds"]["spool"] == 0
    assert pipe["grows"] == sum(1 for v in stats["range_records"] if v) + 1       # a segment a range that completed records, and the join
    assert stats["stream_bytes"] == 2 * room + 4 <= stats["memory_bytes"]
    assert not [n for n in watch.names if ".spool." in n] and len(watch.names) == 2          # the two outputs' temporaries: no spool at any moment
    if range_bytes:
        assert stats["ranges"] > 3


@pytest.mark.parametrize("name", CASES)
def test_beyond_the_budget_the_bam_pipe_is_spooled(want, name, tmp_path):
    from svision_amd import sort
    c = pb.case(name)
    for what, budget in (("a_fifth", want[name, "fixed"][2] // 5), ("one_byte", 1)):
        fifo = pb.Fifo(tmp_path, c["data"])
        out, stats = str(tmp_path / (what + ".bam")), {}
        sort.sort_bam(fifo.path, out, device=DEV, memory_bytes=budget, range_bytes=64 << 10, stats=stats, pipe_bam="stream")
        assert fifo.done() and not fifo.broke
        _same_files(want[name, "fixed"], out)
        pipe = stats["pipe"]
        assert pipe["mode"] == "spooled" and pipe["holds"] == "bam" and pipe["spool_bytes"] > 0 and stats["spans"] > 1
        assert "input" not in stats and stats["records"] == c["n"] and pipe["compressed_bytes"] == len(c["data"])
        assert what != "one_byte" or pipe["grows"] == 0        # (nothing was ever kept)
        for n in os.listdir(str(tmp_path)):
            os.unlink(str(tmp_path / n))


def test_a_header_and_no_record(want, tmp_path):
    from svision_amd import sort
    fifo, stats, out = pb.Fifo(tmp_path, pb.case("none")["data"]), {}, str(tmp_path / "none.bam")
    sort.sort_bam(fifo.path, out, device=DEV, stats=stats, pipe_bam="stream")
    assert fifo.done()
    _same_files(want["none", "fixed"], out)
    assert stats["records"] == 0 and stats["pipe"]["mode"] == "in_core" and stats["pipe"]["holds"] == "bam"


@pytest.mark.parametrize("budget", [None, 1], ids=["in_core", "spooled"])
def test_a_flipped_byte_in_the_third_range(budget, tmp_path):
    """The error names the stream offset of the block; nothing is left behind; the feeding thread has ended although most of the stream
    was never read: the read end was closed."""
    from svision_amd import sort
    data = bytearray(pb.case("hifi")["data"])
    at, n = next((at, n) for at, n in pb.members(bytes(data)) if at > 2 * (64 << 10) + 4096)
    data[at + n // 2] ^= 0x55
    fifo = pb.Fifo(tmp_path, bytes(data))
    before = sorted(os.listdir(str(tmp_path)))
    with pytest.raises(sort.SortWriteError, match=r"the BGZF block at stream offset %d (fails its CRC32|is corrupt)" % at) as exc:
        sort.sort_bam(fifo.path, str(tmp_path / "never.bam"), device=DEV, range_bytes=64 << 10, memory_bytes=budget, pipe_bam="stream")
    assert str(exc.value).startswith(fifo.path + ": ")
    assert sorted(os.listdir(str(tmp_path))) == before
    assert fifo.done() and fifo.broke


def test_a_bam_pipe_among_several_inputs_is_copied_as_it_is(tmp_path):
    """[a.bam, fifo(b.bam)] under "stream" == [a.bam, b.bam]: among several inputs the pipe keeps the copy of its bytes."""
    from svision_amd import sort
    c = pb.case("flush")
    halves = {}
    for k, recs in (("a", c["recs"][:200]), ("b", c["recs"][200:])):
        halves[k] = str(tmp_path / (k + ".bam"))
        htslike.write_bam(halves[k], c["refs"], recs, level=1, policy="stream", header_text=samtext.header_text(c["refs"]), index=False)
    a, b = str(tmp_path / "want.bam"), str(tmp_path / "got.bam")
    sort.sort_bam([halves["a"], halves["b"]], a, device=DEV)
    fifo, stats = pb.Fifo(tmp_path, open(halves["b"], "rb").read()), {}
    sort.sort_bam([halves["a"], fifo.path], b, device=DEV, stats=stats, pipe_bam="stream")
    assert fifo.done() and not fifo.broke
    assert open(a, "rb").read() == open(b, "rb").read() and open(a + ".bai", "rb").read() == open(b + ".bai", "rb").read()
    assert stats["pipe"]["mode"] == "bam_spooled" and stats["pipe"]["holds"] == "bam" and stats["pipe"]["spool_bytes"] == os.path.getsize(halves["b"])
    assert stats["input_records"] == [200, 200] and not [n for n in os.listdir(str(tmp_path)) if ".spool." in n or n.endswith(".tmp")]


def test_the_default_is_the_copy(want, tmp_path, monkeypatch):
    """Without the keyword and the variable, and under "spool", a lone BAM pipe is copied as it is; the variable turns the stream on."""
    from svision_amd import sort
    c = pb.case("stored")
    monkeypatch.delenv("SVX_PIPE_BAM", raising=False)
    for kw, env, mode in (({}, None, "bam_spooled"), ({"pipe_bam": "spool"}, None, "bam_spooled"), ({}, "stream", "in_core")):
        if env:
            monkeypatch.setenv("SVX_PIPE_BAM", env)
        fifo, stats, out = pb.Fifo(tmp_path, c["data"]), {}, str(tmp_path / "out.bam")
        sort.sort_bam(fifo.path, out, device=DEV, stats=stats, **kw)
        assert fifo.done() and stats["pipe"]["mode"] == mode and stats["pipe"]["holds"] == "bam"
        _same_files(want["stored", "fixed"], out)
        for n in os.listdir(str(tmp_path)):
            os.unlink(str(tmp_path / n))
    with pytest.raises(ValueError, match="SVX_PIPE_BAM"):
        sort.sort_bam(c["path"], str(tmp_path / "never.bam"), device=DEV, pipe_bam="sideways")


# ---- the command line (a child process with the BAM on standard input: what the test is about) ----
def test_module_command_line_takes_a_bam_on_standard_input(want, tmp_path):
    c = pb.case("hifi")
    env = {k: v for k, v in os.environ.items() if k not in ("SVX_DEVICE_SORT", "SVX_SORT_TABLES", "SVX_SORT_MEMORY", "SVX_SORT_INDEX", "SVX_PIPE_BAM")}
    out = str(tmp_path / "cli.bam")
    r = subprocess.run([sys.executable, "-m", "svision_amd.sort", "-", "--pipe-bam", "stream", "-o", out], input=c["data"], capture_output=True, timeout=600,
                       env=dict(env, PYTHONPATH=ROOT), cwd=str(tmp_path))
    stdout, stderr = r.stdout.decode(), r.stderr.decode()
    assert r.returncode == 0 and "%d records" % c["n"] in stdout and "<stdin>" in stdout and "of BAM, taken in one pass" in stdout and "kept in core" in stdout, \
        stdout[-2000:] + stderr[-3000:]
    _same_files(want["hifi", "fixed"], out)
