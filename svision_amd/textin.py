"""The inputs of the device sort as its two consumers see them -- ``sort.sort_bam`` (the sorted BAM and its index) and
``ingest_sort.load_sample`` (``SVX_DEVICE_SORT=1``: the sample, no file).  What both do the same way stands here once: how an input is
opened and classified (:func:`open_input`), who owns a pipe's reader and how it is closed (:class:`TextInput`), how a chunk of SAM text
gets into pinned memory (:class:`ChunkReader`) and onto the device (:func:`upload_lines`) -- and nothing of what either does with a
chunk.  No refusal is worded here: a BAM on a pipe is spooled by the one consumer and refused by the other -- unless the switch both
read the same way says "stream" (:func:`pipe_bam_setting`: ``pipe_bam`` / ``SVX_PIPE_BAM``, off by default): then either takes it in one
pass, its header by io.sam.StreamReader.bam_header and its BGZF members by :func:`member_chunks`, the pinned buffers index.stream_ranges
drives the device from.
"""
import os
import stat

import numpy as np

SAM_READ_THREADS = 8                                            # svx_read_range's threads for a chunk of text
DEFAULT_SAM_CHUNK_BYTES = 64 << 20                              # text bytes a chunk of a SAM input (``range_bytes``); see profiles/sort_sam.txt


def input_paths(bam_path):
    """sort_bam's first argument -> the list of paths: a str is one input, a list or tuple several; none: ValueError."""
    if isinstance(bam_path, (str, bytes, os.PathLike)):
        return [os.fsdecode(bam_path)]
    paths = [os.fsdecode(p) for p in bam_path]
    if not paths:
        raise ValueError("sort_bam: an empty list of inputs")
    return paths


def is_stream(path):
    """Whether an input takes the one-pass road: ``-`` (standard input), or a path that is no regular file (a FIFO, /dev/fd/N) --
    decided by os.stat, before a byte is read."""
    if path == "-":
        return True
    try:
        return not stat.S_ISREG(os.stat(path).st_mode)
    except OSError:
        return False                                            # (the file road names what is wrong with the path)


def name_of(path):
    """What messages call an input: its path, ``<stdin>`` for ``-``."""
    from .io import sam
    return sam.STREAM_NAME if path == "-" else path


class TextInput:
    """One input, opened: ``kind`` ("bam", "sam": text in a regular file, "pipe": read once), ``path``, the ``name`` messages call it,
    ``peek_kind``: what its first bytes hold (io.sam.stream_kind), ``reader``: a pipe's io.sam.StreamReader; of SAM text ``text``: the
    ``@`` lines' bytes, ``first``: (the bytes, the lines) in front of the first alignment line, ``headerless``: no @SQ line."""

    def __init__(self, kind, path, peek_kind, text=b"", reader=None):
        self.kind, self.path, self.name, self.peek_kind, self.text, self.reader = kind, path, name_of(path), peek_kind, text, reader
        self.first = (len(text), text.count(b"\n"))
        self.headerless = not any(l.startswith(b"@SQ\t") for l in text.split(b"\n"))

    def close(self, failed=False):
        """A pipe's reader ended and its descriptor closed; ``failed``: standard input is pointed at the null device, so that the
        writer of the pipe ends with EPIPE and does not block."""
        if self.reader is not None:
            self.reader.close()
        if failed and self.path == "-":
            null = os.open(os.devnull, os.O_RDONLY)
            os.dup2(null, 0)
            os.close(null)


def open_input(path):
    """An input opened, classified and -- SAM text -- its header read -> TextInput: a regular file is "sam" or "bam" by its first MB, any
    other path a "pipe" whatever it holds.  OSError, io.sam.SamError: it is closed as after a failure, the caller words the message."""
    from .io import sam
    if not is_stream(path):
        with open(path, "rb") as f:
            peek_kind = sam.stream_kind(f.read(1 << 20))
        return TextInput("sam", path, peek_kind, sam.header_end(path)) if peek_kind == sam.STREAM_SAM else TextInput("bam", path, peek_kind)
    reader = sam.StreamReader(0 if path == "-" else os.open(path, os.O_RDONLY), own=path != "-")
    try:
        peek_kind = sam.stream_kind(reader.peek())
        return TextInput("pipe", path, peek_kind, reader.header() if peek_kind == sam.STREAM_SAM else b"", reader)
    except BaseException:
        TextInput("pipe", path, None, reader=reader).close(failed=True)
        raise


class ReadError(OSError):
    """A chunk of the file ``path`` could not be read whole -- ``what``: the reader's words; as a string "path: what"."""

    def __init__(self, path, what):
        OSError.__init__(self, "%s: %s" % (path, what))
        self.path, self.what = path, what


class Chunk:
    """A chunk of text: ``data``, its ``n`` bytes -- a NumPy view that the next chunk overwrites --, ``pinned``: the buffer they lie in,
    ``line_no``: the input's lines in front of it, ``place``: (file offset, n), ``n_lines``: its lines once :func:`upload_lines` ran."""
    __slots__ = ("data", "pinned", "n", "line_no", "place", "n_lines")

    def __init__(self, data, pinned, n, line_no, place):
        self.data, self.pinned, self.n, self.line_no, self.place, self.n_lines = data, pinned, n, line_no, place, None


class ChunkReader:
    """The chunks of text inputs, and the pinned buffers they are read into.  ``read(path, file offset, n, NumPy view) -> the bytes
    read``, raising OSError (default: svx_read_range with SAM_READ_THREADS) and ``alloc(n) -> a buffer with .numpy(), or a NumPy array`` (default: a
    pinned uint8 tensor) can be handed in: the class then runs without a device.  ``clock.lap("read", False)`` closes every read."""

    def __init__(self, torch, lib, clock, read=None, alloc=None):
        def read_range(path, at, n, view):
            if lib.svx_read_range(path.encode(), at, n, view.ctypes.data, SAM_READ_THREADS) != 0:
                raise ReadError(path, lib.svx_bam_error().decode())
            return n
        self.clock, self.read, self.buf, self.pinned = clock, read or read_range, None, None
        self.alloc = alloc or (lambda n: torch.empty(n, dtype=torch.uint8, pin_memory=True))

    def _buffer(self, n):
        t = self.alloc(n)
        return (t.numpy() if hasattr(t, "numpy") else t), t     # the buffer's NumPy view, and the buffer

    def at(self, inp, place, line_no=0):
        """The chunk at ``place`` (file offset, bytes) of a regular file, read whole (or ReadError) into the one buffer, which grows."""
        at, n = place
        if self.buf is None or self.buf.size < n:
            self.buf, self.pinned = self._buffer(n)
        got = self.read(inp.path, at, n, self.buf[:n])
        if got != n:
            raise ReadError(inp.path, "%d of the %d bytes at file offset %d read" % (got, n, at))
        self.clock.lap("read", False)
        return Chunk(self.buf[:n], self.pinned, n, line_no, place)

    def chunks(self, inp, step=None):
        """Generator: the text of ``inp`` behind its header in chunks of ``step`` bytes (default DEFAULT_SAM_CHUNK_BYTES) cut at line
        ends, a longer line growing its chunk -- a file's by io.sam.chunk_places; a pipe's by StreamReader.chunks, whose thread fills
        pinned buffers ahead of the caller.  A chunk is the caller's until it asks for the next one."""
        from .io import sam
        step = step or DEFAULT_SAM_CHUNK_BYTES
        at, line_no = inp.first
        if inp.reader is None:
            for place in sam.chunk_places(inp.path, at, step):
                chunk = self.at(inp, place, line_no)
                yield chunk
                if chunk.n_lines is None:                       # (svx_sam_lines' count where the caller took it: no second count on the host)
                    chunk.n_lines = int(np.count_nonzero(chunk.data == 10)) + bool(chunk.data[-1] != 10)
                line_no += chunk.n_lines
            return
        pinned = {}

        def alloc(n):                                           # a pinned buffer as the reader takes it: its NumPy view
            a, t = self._buffer(n)
            pinned[a.ctypes.data] = t
            return a
        for buf, n, line_no in inp.reader.chunks(step, line_no, alloc):
            self.clock.lap("read", False)
            yield Chunk(buf[:n], pinned[buf.ctypes.data], n, line_no, (at, n))
            at += n


PIPE_BAM = ("spool", "stream")                                  # SVX_PIPE_BAM / ``pipe_bam``: a BAM on a pipe copied into a file first, or taken in one pass
# Compressed bytes a chunk of a BAM on a pipe: the text chunk's size, not a file range's (ingest_gpu.LARGE_GROUP_BYTES) -- two pinned
# buffers of it are held, and the device starts on the aligner's output a chunk behind it.  The one size measured: profiles/pipe_bam.txt
DEFAULT_PIPE_BAM_BYTES = 64 << 20


def pipe_bam_setting(pipe_bam, consumer):
    """``pipe_bam`` as a consumer was handed it (None: ``SVX_PIPE_BAM`` of the environment) -> whether a BAM on a pipe is streamed.  Unset,
    empty, "0" or "spool": the consumer's road of today; anything but those and "stream": ValueError."""
    value = os.environ.get("SVX_PIPE_BAM") if pipe_bam is None else pipe_bam
    if value in (None, "", "0") or value in PIPE_BAM:
        return value == "stream"
    raise ValueError("%s: pipe_bam (SVX_PIPE_BAM) is %r, none of %s" % (consumer, value, ", ".join(PIPE_BAM)))


def member_chunks(torch, inp, range_bytes=None):
    """The BGZF members of a BAM pipe behind its header (io.sam.StreamReader.bam_header has run) in chunks of ``range_bytes``
    compressed bytes (default DEFAULT_PIPE_BAM_BYTES), read by the reader's thread into pinned buffers -> what index.stream_ranges takes."""
    def alloc(n):                                               # (the NumPy view keeps its pinned tensor alive)
        return torch.empty(n, dtype=torch.uint8, pin_memory=True).numpy()
    return inp.reader.member_chunks(range_bytes or DEFAULT_PIPE_BAM_BYTES, alloc)


def upload_lines(torch, kernels, dev, clock, chunk):
    """A chunk uploaded with the kernels' slack behind it, zeroed, and its line table -> (d_text, d_line_off, the number of lines)."""
    d_text = torch.empty(chunk.n + kernels.SAM_SLACK, dtype=torch.uint8, device=dev)
    d_text[:chunk.n].copy_(chunk.pinned[:chunk.n], non_blocking=True)
    d_text[chunk.n:] = 0
    clock.lap("upload")
    d_line_off, chunk.n_lines = kernels.sam_lines(d_text, chunk.n)
    clock.lap("lines")
    return d_text, d_line_off, chunk.n_lines


def line_bytes(data, line_off, i):
    """Line ``i`` of a chunk (``data``: its bytes, ``line_off`` [lines + 1]: the lines' offsets) without its newline."""
    line = data[int(line_off[i]):int(line_off[i + 1])].tobytes()
    return line[:-1] if line.endswith(b"\n") else line


def line_refusal(line, tid_of, line_no, kernel, code):
    """What to say of line ``line_no`` that ``kernel`` refused with ``code``: the words of the host statement of the rules."""
    from .io import sam
    try:
        sam.encode_line(line, tid_of)
    except sam.SamError as exc:
        return str(exc.at(line_no))
    return "line %d: not an alignment line (%s: %d)" % (line_no, kernel, code)
