"""svision_amd/textin.py without a GPU: what sort_bam and load_sample share about their inputs.  The chunk reader runs over a NumPy
allocator and an ``os.preadv`` read; pipes are ``os.pipe()`` ends that a thread feeds, handed in as /dev/fd/N.  Expected values come
from the text itself."""
import gzip
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from svision_amd import textin
from svision_amd.io import sam
from tests import htslike
from tests.test_sort_steps_cpu import host_clock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrA\tLN:100000\n@SQ\tSN:chrB\tLN:50000\n@PG\tID:aligner\n"
NO_SQ = b"@HD\tVN:1.6\n@CO\tno dictionary\n"


def _line(i, seq=b"ACGT"):
    return b"r%d\t0\tchr%c\t%d\t60\t%dM\t*\t0\t0\t%s\t%s\n" % (i, b"AB"[i % 2], 1 + 37 * i, len(seq), seq, b"I" * len(seq))


SHORT = [_line(i) for i in range(300)]
LONG = _line(1000, b"ACGT" * 1300)                               # 10 KB: longer than either step
TEXTS = {"short_lines": HEADER + b"".join(SHORT),
         "long_line_in_the_middle": HEADER + b"".join(SHORT[:40]) + LONG + b"".join(SHORT[40:80]),
         "long_line_first": HEADER + LONG + b"".join(SHORT[:40]),
         "no_last_newline": HEADER + b"".join(SHORT[:50])[:-1],
         "header_only": HEADER,
         "no_header": b"".join(SHORT[:60])}


def _preadv(path, at, n, view):
    fd = os.open(path, os.O_RDONLY)
    try:
        return os.preadv(fd, [view], at)
    finally:
        os.close(fd)


def _reader():
    return textin.ChunkReader(None, None, host_clock(), read=_preadv, alloc=lambda n: np.empty(n, np.uint8))


class _Piped:
    """``data`` on a pipe that a thread feeds: ``path`` is /dev/fd/N of the read end, which ``close`` gives up."""

    def __init__(self, data):
        self.r, w = os.pipe()
        self.path = "/dev/fd/%d" % self.r

        def feed():
            try:
                for at in range(0, len(data), 4096):
                    os.write(w, data[at:at + 4096])
            except BrokenPipeError:
                pass
            finally:
                os.close(w)
        self.thread = threading.Thread(target=feed, daemon=True)
        self.thread.start()

    def close(self):
        os.close(self.r)
        self.thread.join(20)
        assert not self.thread.is_alive()


def _header_of(text):
    return b"".join(l for l in text.splitlines(True) if l.startswith(b"@"))


@pytest.mark.parametrize("step", [64, 2048])
@pytest.mark.parametrize("name", list(TEXTS))
def test_a_file_and_a_pipe_give_the_same_chunks(tmp_path, name, step):
    text = TEXTS[name]
    header = _header_of(text)
    path = str(tmp_path / "in.sam")
    with open(path, "wb") as f:
        f.write(text)
    inp, reader = textin.open_input(path), _reader()
    assert (inp.kind, inp.text, inp.first, inp.reader) == ("sam", header, (len(header), header.count(b"\n")), None)
    from_file, places = [], []
    for chunk in reader.chunks(inp, step):
        assert chunk.n == len(chunk.data) and chunk.pinned is reader.pinned and chunk.place[1] == chunk.n
        from_file.append((chunk.data.tobytes(), chunk.line_no))
        places.append(chunk.place)
    piped = _Piped(text)
    inp_pipe = textin.open_input(piped.path)
    try:
        assert (inp_pipe.kind, inp_pipe.peek_kind, inp_pipe.text, inp_pipe.first) == ("pipe", sam.STREAM_SAM, header, inp.first)
        from_pipe = [(c.data.tobytes(), c.line_no, c.place) for c in _reader().chunks(inp_pipe, step)]
    finally:
        inp_pipe.close()
        piped.close()
    assert [c[:2] for c in from_pipe] == from_file and [c[2] for c in from_pipe] == places
    assert b"".join(c for c, _no in from_file) == text[len(header):]
    lines = header.count(b"\n")
    for k, (c, line_no) in enumerate(from_file):
        assert line_no == lines and (c.endswith(b"\n") or k == len(from_file) - 1)
        assert len(c) <= step or c[:-1].count(b"\n") == 0          # (as long as the step allows, unless one line is longer)
        lines += c.count(b"\n") + (not c.endswith(b"\n"))
    assert [at for at, _n in places] == [len(header) + sum(n for _at, n in places[:k]) for k in range(len(places))]
    # ---- every place once more, in another order, through the one buffer
    for place, (c, _no) in reversed(list(zip(places, from_file))):
        again = reader.at(inp, place)
        assert again.data.tobytes() == c and again.place == place
    if places:
        with open(path, "wb") as f:
            f.write(text[:places[-1][0] + places[-1][1] - 1])       # the file a byte shorter: the last place cannot be read whole
        with pytest.raises(textin.ReadError, match="in.sam: "):
            reader.at(inp, places[-1])


def test_the_buffer_grows_with_a_long_line_and_is_kept(tmp_path):
    path = str(tmp_path / "in.sam")
    with open(path, "wb") as f:
        f.write(TEXTS["long_line_in_the_middle"])
    allocated = []
    reader = textin.ChunkReader(None, None, host_clock(), read=_preadv, alloc=lambda n: (allocated.append(n), np.empty(n, np.uint8))[1])
    chunks = [c.n for c in reader.chunks(textin.open_input(path), 2048)]
    assert max(chunks) == len(LONG) and allocated == [chunks[0], len(LONG)]       # one buffer, grown once: no allocation a chunk


def test_open_input_says_what_a_file_holds(tmp_path):
    def opened(name, data):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(data)
        return textin.open_input(path)
    inp = opened("a.sam", TEXTS["short_lines"])
    assert (inp.kind, inp.peek_kind, inp.name, inp.first, inp.headerless) == ("sam", sam.STREAM_SAM, inp.path, (len(HEADER), 4), False)
    inp = opened("b.sam", NO_SQ + SHORT[0])
    assert (inp.kind, inp.text, inp.first, inp.headerless) == ("sam", NO_SQ, (len(NO_SQ), 2), True)
    inp = opened("c.sam", SHORT[0])
    assert (inp.kind, inp.text, inp.first, inp.headerless) == ("sam", b"", (0, 0), True)
    inp = textin.open_input(os.path.join(ROOT, "tests", "golden", "ont_small.bam"))
    assert (inp.kind, inp.peek_kind, inp.text, inp.reader) == ("bam", sam.STREAM_BAM, b"", None)
    inp = opened("d.sam.gz", gzip.compress(TEXTS["short_lines"]))
    assert (inp.kind, inp.peek_kind, inp.text) == ("bam", sam.STREAM_GZIP, b"")      # (what to do with it is the consumer's decision)
    inp.close(failed=True)                                      # (a file: nothing to close, and no descriptor is touched)
    with pytest.raises(OSError):
        textin.open_input(str(tmp_path / "missing.sam"))


@pytest.mark.parametrize("what", ["empty", "sam", "bam", "gzip"])
def test_open_input_says_what_a_pipe_holds(what):
    bam_bytes = htslike._bgzf_block(sam.bam_header_bytes(sam.parse_header(HEADER)), 1) + htslike.EOF_BLOCK
    data, kind, text = {"empty": (b"", sam.STREAM_EMPTY, b""), "sam": (TEXTS["short_lines"], sam.STREAM_SAM, HEADER),
                        "bam": (bam_bytes, sam.STREAM_BAM, b""), "gzip": (gzip.compress(TEXTS["short_lines"]), sam.STREAM_GZIP, b"")}[what]
    piped = _Piped(data)
    try:
        assert textin.is_stream(piped.path) and textin.is_stream("-") and textin.name_of("-") == sam.STREAM_NAME
        inp = textin.open_input(piped.path)
        assert (inp.kind, inp.peek_kind, inp.text, inp.name) == ("pipe", kind, text, piped.path) and inp.reader is not None
        assert inp.first == (len(text), text.count(b"\n")) and inp.headerless == (what != "sam")
        fd = inp.reader.fd
        inp.close()
        with pytest.raises(OSError):
            os.fstat(fd)                                        # the reader's own descriptor is closed: the writer ends with EPIPE
    finally:
        piped.close()


CHILD = r"""
import os, stat, sys
from svision_amd import textin
path = sys.argv[1]
if path != "-":                                                 # a FIFO with some text in it (opened for both ends: nothing blocks)
    os.mkfifo(path)
    w = os.open(path, os.O_RDWR)
    os.write(w, sys.argv[2].encode())
ident = lambda st: (st.st_dev, st.st_ino, st.st_rdev)
before, null = ident(os.fstat(0)), ident(os.stat(os.devnull))
inp = textin.open_input(path)
fd = inp.reader.fd
inp.close(failed=True)
try:
    os.fstat(fd)
    closed = False
except OSError:
    closed = True
after = ident(os.fstat(0))
print(inp.peek_kind, inp.first[1], fd, closed, after == null, after == before, before == null)
"""


def test_a_failed_close_points_standard_input_at_the_null_device(tmp_path):
    """In a child process, so that the descriptor 0 that changes is not the test runner's."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD, "-"], input=TEXTS["short_lines"], capture_output=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout.decode().split() == ["sam", "4", "0", "False", "True", "False", "False"]       # descriptor 0 open, and the null device now
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "fifo"), TEXTS["short_lines"][:4000].decode()], input=b"untouched",
                       capture_output=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    kind, lines, fd, closed, is_null, same, was_null = r.stdout.decode().split()
    assert (kind, lines, closed, is_null, same, was_null) == ("sam", "4", "True", "False", "True", "False") and int(fd) > 2


def test_line_bytes():
    lines = [b"first\tline", b"", b"the middle one", b"last"]
    for tail in (b"\n", b""):
        data = np.frombuffer(b"\n".join(lines) + tail, np.uint8)
        line_off = np.cumsum([0] + [len(l) + 1 for l in lines])
        line_off[-1] = data.size
        assert [textin.line_bytes(data, line_off, i) for i in range(len(lines))] == lines
    tid_of = sam.tid_table(["chrA", "chrB"])
    assert textin.line_refusal(SHORT[3][:-1], tid_of, 9, "svx_sam_measure", -7) == "line 9: not an alignment line (svx_sam_measure: -7)"
    assert textin.line_refusal(SHORT[3][:-1].replace(b"chrB", b"chrZ"), tid_of, 9, "svx_sam_measure", -7).startswith("line 9: ")
