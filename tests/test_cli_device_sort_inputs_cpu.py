"""The input step of svision_amd.cli.run without a device: under SVX_DEVICE_SORT=1 standard input, a comma list and SAM text reach
cli._load_unsorted (patched here); in a run of two ranks each is refused before the device or the process group is touched; with
the switch unset the three refusals read as they did.  A path that is no regular file is a pipe: no byte of it is read in front of
the loader, and a refusal leaves it unopened."""
import os

import pytest
import torch

from svision_amd import cli, sample as _sample
from svision_amd.io import bam
from tests import helpers, samtext, sortcases
from tests.test_cli_stages_cpu import _file_options, _logs, _no_device, _root_handlers


class _Reached(Exception):
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(the shuffled collect_small, the same records as SAM text, its FASTA as a file)."""
    d = tmp_path_factory.mktemp("cli_inputs")
    shuffled, _sorted_path, _want = sortcases.shuffled_files(os.path.join(helpers.GOLDEN, "collect_small.bam"), d, 21)
    table = bam.read_bam(shuffled, with_seq=True)
    text = str(d / "collect_small.sam")
    with open(text, "wb") as f:
        f.write(samtext.text(list(zip(table.references, table.lengths)), samtext.records_of_table(table), header=table.header_text))
    fasta = helpers.load_golden_fasta()
    fa = str(d / "collect_small.fa")
    bam.write_fasta(fa, {n: fasta._seq[n] for n in fasta.references})
    return shuffled, text, fa


def _inputs(files):
    shuffled, text, _fa = files
    return [("stdin", "-", None, "stdin"), ("list", shuffled + "," + text, [shuffled, text], shuffled), ("text", text, None, text)]


def _clean(monkeypatch, **env):
    for k in ("SVX_DEVICE_SORT", "SVX_BUILD_INDEX", "WORLD_SIZE", "RANK"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_under_the_switch_each_reaches_the_loader(files, tmp_path, monkeypatch):
    _clean(monkeypatch, SVX_DEVICE_SORT="1")
    _no_device(monkeypatch)
    for name, value, several, registered in _inputs(files):
        seen = []

        def load(options, several_=None):
            seen.append((options.bam_path, several_))
            return _Sample()
        monkeypatch.setattr(cli, "_load_unsorted", load)
        monkeypatch.setattr(cli, "_plan", lambda *a, **kw: (_ for _ in ()).throw(_Reached(name)))
        before = _root_handlers()
        with pytest.raises(_Reached):
            cli.run(_file_options(tmp_path / name, value, files[2]))
        assert seen == [(value, several)] and _root_handlers() == before
        assert isinstance(_sample._CACHE.get(("registered", registered)), _Sample), name
        assert not [f for f in os.listdir(str(tmp_path / name)) if f.endswith((".bam", ".bai"))]


class _Table:
    references, lengths = ["chrA"], [10]


class _Sample:
    fasta, table = None, _Table()


def test_two_ranks_are_refused_before_the_device(files, tmp_path, monkeypatch):
    _clean(monkeypatch, SVX_DEVICE_SORT="1", WORLD_SIZE="2", RANK="0")
    _no_device(monkeypatch)
    monkeypatch.setattr(cli, "_load_unsorted", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("a refused run reached the loader")))
    for name, value, _several, _registered in _inputs(files):
        before = _root_handlers()
        with pytest.raises(SystemExit) as exit_:
            cli.run(_file_options(tmp_path / name, value, files[2]))
        assert exit_.value.code == 1 and _root_handlers() == before
        (text,) = _logs(str(tmp_path / name)).values()
        assert "SVX_DEVICE_SORT=1 sorts an unsorted BAM in a single-rank run only" in text and text.count("[ERROR") == 1, text


def test_without_the_switch_the_refusals_read_as_they_did(files, tmp_path, monkeypatch):
    _clean(monkeypatch)
    _no_device(monkeypatch)
    monkeypatch.setattr(cli, "_load_unsorted", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("a refused run reached the loader")))
    for name, value, _several, _registered in _inputs(files):
        before = _root_handlers()
        if name == "text":                                      # SAM text is read as a BAM, which it is not: the reader's own words
            with pytest.raises(ValueError, match="not a BGZF block") as refused:
                cli.run(_file_options(tmp_path / name, value, files[2]))
            assert str(refused.value) == value + ": not a BGZF block" and not isinstance(refused.value, SystemExit)
            assert _root_handlers() == before
            continue
        with pytest.raises(SystemExit) as exit_:
            cli.run(_file_options(tmp_path / name, value, files[2]))
        assert exit_.value.code == 1 and _root_handlers() == before
        errors = [l for text in _logs(str(tmp_path / name)).values() for l in text.splitlines() if "[ERROR" in l]
        assert len(errors) == 1 and ("SVX_DEVICE_SORT=write" if name == "stdin" else "python -m svision_amd.sort") in errors[0], errors
    assert not torch.distributed.is_initialized()


# ---- a path that is no regular file is a pipe: no byte of it is read in front of the loader ----
class _Writer:
    """A FIFO and a thread that writes ``data`` into it once a reader has opened it."""

    def __init__(self, d, data):
        import threading
        self.path, self.data, self.opened = os.path.join(str(d), "aligner.fifo"), data, threading.Event()
        os.mkfifo(self.path)
        self.thread = threading.Thread(target=self._feed, daemon=True)
        self.thread.start()

    def _feed(self):
        try:
            with open(self.path, "wb") as f:                    # (blocks until somebody opens the FIFO to read)
                self.opened.set()
                f.write(self.data)
        except BrokenPipeError:
            pass

    def end(self):
        """-> whether anybody had opened the pipe to read.  Where nobody had, the writer is released by a reader that opens and closes."""
        taken = self.opened.is_set()
        if not taken:
            fd = os.open(self.path, os.O_RDONLY | os.O_NONBLOCK)
            assert self.opened.wait(10)
            os.close(fd)
        self.thread.join(10)
        assert not self.thread.is_alive()
        os.unlink(self.path)
        return taken


def test_a_fifo_is_not_read_in_front_of_the_loader(files, tmp_path, monkeypatch):
    text = open(files[1], "rb").read()
    _no_device(monkeypatch)
    # under the switch: the loader gets the path, and every byte is still in the pipe
    _clean(monkeypatch, SVX_DEVICE_SORT="1")
    w, got = _Writer(tmp_path, text), []

    def load(options, several_=None):
        with open(options.bam_path, "rb") as f:
            got.append(f.read())
        return _Sample()
    monkeypatch.setattr(cli, "_load_unsorted", load)
    monkeypatch.setattr(cli, "_plan", lambda *a, **kw: (_ for _ in ()).throw(_Reached("fifo")))
    with pytest.raises(_Reached):
        cli.run(_file_options(tmp_path / "fifo_1", w.path, files[2]))
    assert got == [text] and w.end() and isinstance(_sample._CACHE.get(("registered", w.path)), _Sample)
    # two ranks, and the switch unset: refused in one line, and nobody has opened the pipe
    monkeypatch.setattr(cli, "_load_unsorted", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("a refused run reached the loader")))
    for name, env, message in (("fifo_ranks", dict(SVX_DEVICE_SORT="1", WORLD_SIZE="2", RANK="0"), "SVX_DEVICE_SORT=1 sorts an unsorted BAM in a single-rank run only"),
                               ("fifo_unset", {}, "SVX_DEVICE_SORT=write")):
        _clean(monkeypatch, **env)
        w = _Writer(tmp_path, text)
        with pytest.raises(SystemExit) as exit_:
            cli.run(_file_options(tmp_path / name, w.path, files[2]))
        assert exit_.value.code == 1 and not w.end()
        (log,) = _logs(str(tmp_path / name)).values()
        assert message in log and w.path in log and log.count("[ERROR") == 1, log
