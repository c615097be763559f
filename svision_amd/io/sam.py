"""SAM text -> the BAM record bytes htslib writes for it (``sam_parse1`` + ``bam_write1``): the host statement of the rules the
device parser (svision_amd/csrc/svx_sam_core.hpp) follows, the road of every line that parser hands back (``SVX_SAM_HOST``), and the
yardstick of its CPU model (tools/hostwave/sam_main.cpp).  Pure Python + ``struct``.  At the end of the file: :class:`StreamReader`,
the text of a pipe read once -- its first bytes, its header, its chunks filled by a thread of their own (host only, no torch) --, and
the same for a BAM that arrives there: its header through zlib (:meth:`StreamReader.bam_header`) and its bytes in chunks of whole BGZF
members (:meth:`StreamReader.member_chunks`).

The header.  The ``@`` lines in front of the first record are the BAM header's text, byte for byte; the reference dictionary is
the ``@SQ`` lines' ``SN`` / ``LN`` in order.  No ``@SQ`` line: SamError.  An ``@`` line behind a record: SamError.

A record line.  Lines end at ``\\n``, the last one may lack it; a ``\\r`` belongs to the last field.  Eleven tab-separated fields
and any number of tags:

  QNAME   l_read_name = its bytes + one NUL, no padding; empty or more than 254 bytes: error
  FLAG    decimal, 0 .. 65535
  RNAME   ``*`` -> -1; else the @SQ line's index; a name no @SQ line has: error (htslib warns and unmaps)
  POS     decimal 0 .. 2^31 - 1, stored minus 1
  MAPQ    decimal, 0 .. 255
  CIGAR   ``*`` -> no operation; else <length><one of MIDNSHP=X> repeated, a length of 1 to 9 digits below 2^28.  More than 65,535
          operations: the record carries ``<l_seq>S<span>N`` and the real words go behind the line's own tags as CG:B,I (SAMv1 4.2.2)
  RNEXT   ``=`` -> the record's own tid, ``*`` -> -1, else as RNAME
  PNEXT   as POS
  TLEN    decimal with an optional ``-``, within +-(2^31 - 1)
  SEQ     ``*`` -> l_seq 0; else 4 bits a base by the table ``=ACMGRSVTWYHKDBN``, either case, any other byte N, the first base in the
          high nibble, an odd length leaves a zero low nibble
  QUAL    ``*`` -> 0xFF x l_seq; else every byte minus 33, as many as l_seq or: error
  bin     reg2bin(pos, pos + max(reference span, 1)) (the span: the lengths of M D N = X), 4680 where tid is -1; 16 bits
  tags    ``XX:T:value``.  A: one byte.  Z and H: the bytes + NUL.  i: the narrowest type, htslib's choice -- negative: c, s, i;
          else C, S, I; outside [-2^31, 2^32): error.  f: float32(double(text)), the decimal -> double conversion correctly rounded
          (``strtod``, Python's ``float``).  B: ``B:<cCsSiIf>`` and a value behind every comma (none: an empty array); integers
          within the subtype's range, floats as ``f``

Errors raise :class:`SamError` (a ValueError) whose message names the 1-based line number and whose ``code`` is the device
parser's code for the same line (include/svx.h, SVX_SAM_E_*)."""
import collections
import os
import queue
import re
import select
import struct
import threading
import time
import zlib

HOST = -1                                                       # SVX_SAM_HOST: valid as far as seen, not taken by the kernels
E_FIELDS, E_NUMBER, E_NAME, E_RNAME, E_CIGAR, E_QUAL, E_TAG, E_RANGE, E_HEADER = -2, -3, -4, -5, -6, -7, -8, -9, -10
CIGAR_OPS = b"MIDNSHP=X"
MAX_CIGAR_OPS = 65535

_BASE = bytearray([15] * 256)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    _BASE[_c] = _i
    _BASE[ord(chr(_c).lower())] = _i
_HI = bytes(b << 4 for b in _BASE)
_LO = bytes(_BASE)
_QUAL = bytes((b - 33) & 255 for b in range(256))
_OP = {c: i for i, c in enumerate(CIGAR_OPS)}
_REF_OPS = frozenset(b"MDN=X")
_CIGAR_RE = re.compile(rb"(\d{1,9})([MIDNSHP=X])")
_FLOAT_RE = re.compile(rb"[+-]?(?:(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?|inf|infinity|nan)\Z", re.I)
_INT_RE = re.compile(rb"-?\d{1,11}\Z")
_B_TYPES = {ord("c"): ("b", -128, 127), ord("C"): ("B", 0, 255), ord("s"): ("h", -32768, 32767), ord("S"): ("H", 0, 65535),
            ord("i"): ("i", -(1 << 31), (1 << 31) - 1), ord("I"): ("I", 0, (1 << 32) - 1)}

SamHead = collections.namedtuple("SamHead", "references lengths text sort_order")


class SamError(ValueError):
    def __init__(self, message, code, line=None):
        ValueError.__init__(self, message if line is None else "line %d: %s" % (line, message))
        self.what, self.code, self.line = message, code, line

    def at(self, line):
        return SamError(self.what, self.code, line)


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def _int(text, lo, hi, what, range_code=E_NUMBER):
    if not _INT_RE.match(text):
        raise SamError("%s is not a number: %r" % (what, text[:20]), E_NUMBER)
    v = int(text)
    if not lo <= v <= hi:
        raise SamError("%s %d lies outside [%d, %d]" % (what, v, lo, hi), range_code)
    return v


def _float(text):
    if not _FLOAT_RE.match(text):
        raise SamError("not a floating-point value: %r" % text[:20], E_NUMBER)
    return float(text)


def _ref(name, tid_of):
    if name == b"*":
        return -1
    tid = tid_of.get(name)
    if tid is None:
        raise SamError("the reference %r is in no @SQ line" % name[:40].decode("latin-1"), E_RNAME)
    return tid


def encode_tag(field):
    """One tag field ``XX:T:value`` -> its BAM bytes."""
    if len(field) < 5 or field[2] != 58 or field[4] != 58:
        raise SamError("a malformed tag: %r" % field[:20], E_TAG)
    name, typ, value = field[:2], field[3:4], field[5:]
    if typ == b"A":
        if len(value) != 1:
            raise SamError("an A tag of %d bytes" % len(value), E_TAG)
        return name + b"A" + value
    if typ in (b"Z", b"H"):
        return name + typ + value + b"\0"
    if typ == b"i":
        v = _int(value, -(1 << 31), (1 << 32) - 1, "an integer tag", E_RANGE)
        if v < 0:
            t = "cb" if v >= -128 else "sh" if v >= -32768 else "ii"
        else:
            t = "CB" if v <= 255 else "SH" if v <= 65535 else "II"
        return name + t[:1].encode() + struct.pack("<" + t[1], v)
    if typ == b"f":
        return name + b"f" + struct.pack("<f", _float(value))
    if typ == b"B":
        if not value or (len(value) > 1 and value[1] != 44):
            raise SamError("a malformed B tag: %r" % field[:20], E_TAG)
        sub = value[0]
        items = value[2:].split(b",") if len(value) > 1 else []
        if sub == ord("f"):
            return name + b"Bf" + struct.pack("<i%df" % len(items), len(items), *[_float(x) for x in items])
        if sub not in _B_TYPES:
            raise SamError("a B tag of subtype %r" % chr(sub), E_TAG)
        fmt, lo, hi = _B_TYPES[sub]
        return name + b"B" + value[:1] + struct.pack("<i%d%s" % (len(items), fmt), len(items), *[_int(x, lo, hi, "an array value") for x in items])
    raise SamError("a tag of type %r" % typ.decode("latin-1"), E_TAG)


def cigar_words(text):
    """CIGAR text (not ``*``) -> (the BAM words, the reference span)."""
    words, span, at = [], 0, 0
    for m in _CIGAR_RE.finditer(text):
        if m.start() != at:
            break
        at = m.end()
        n = int(m.group(1))
        if n >= 1 << 28:
            raise SamError("a CIGAR length of %d" % n, E_CIGAR)
        op = m.group(2)[0]
        words.append(n << 4 | _OP[op])
        if op in _REF_OPS:
            span += n
    if at != len(text) or not words:
        raise SamError("a malformed CIGAR near %r" % text[at:at + 12], E_CIGAR)
    return words, span


def fields_of(line, tid_of):
    """One alignment line -> (tid, pos, flag, reference span): the sort key and the index's fields.  Checks the core fields only."""
    f = line.split(b"\t", 6)
    if len(f) < 7:
        raise SamError("fewer than 11 fields", E_FIELDS)
    return (_ref(f[2], tid_of), _int(f[3], 0, (1 << 31) - 1, "POS") - 1, _int(f[1], 0, 65535, "FLAG"),
            0 if f[5] == b"*" else cigar_words(f[5])[1])


def encode_line(line, tid_of):
    """One alignment line (no ``\\n``) and {reference name (bytes): tid} -> the line's BAM record including its ``block_size``."""
    if line[:1] == b"@":
        raise SamError("a header line behind the first record", E_HEADER)
    f = line.split(b"\t")
    if len(f) < 11:
        raise SamError("an empty line" if not line else "%d fields, an alignment has at least 11" % len(f), E_FIELDS)
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if not qname or len(qname) > 254:
        raise SamError("a read name of %d bytes" % len(qname), E_NAME)
    flag = _int(flag, 0, 65535, "FLAG")
    tid = _ref(rname, tid_of)
    pos = _int(pos, 0, (1 << 31) - 1, "POS") - 1
    mapq = _int(mapq, 0, 255, "MAPQ")
    words, span = ([], 0) if cigar == b"*" else cigar_words(cigar)
    next_tid = tid if rnext == b"=" else _ref(rnext, tid_of)
    next_pos = _int(pnext, 0, (1 << 31) - 1, "PNEXT") - 1
    tlen = _int(tlen, -(1 << 31) + 1, (1 << 31) - 1, "TLEN")
    if seq == b"*":
        l_seq, packed = 0, b""
    else:
        l_seq = len(seq)
        hi, lo = seq[0::2].translate(_HI), seq[1::2].translate(_LO).ljust((l_seq + 1) // 2, b"\0")
        packed = (int.from_bytes(hi, "little") | int.from_bytes(lo, "little")).to_bytes(len(hi), "little")      # (a bytewise OR)
    if qual == b"*":
        q = b"\xff" * l_seq
    elif len(qual) != l_seq:
        raise SamError("%d quality values for %d bases" % (len(qual), l_seq), E_QUAL)
    else:
        q = qual.translate(_QUAL)
    tags = b"".join(encode_tag(t) for t in f[11:])
    if len(words) > MAX_CIGAR_OPS:
        tags += b"CGBI" + struct.pack("<i%dI" % len(words), len(words), *words)
        words = [l_seq << 4 | 4, span << 4 | 3]
    bin_ = reg2bin(pos, pos + max(span, 1)) & 0xFFFF if tid >= 0 else 4680
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(qname) + 1, mapq, bin_, len(words), flag, l_seq, next_tid, next_pos, tlen) \
        + qname + b"\0" + struct.pack("<%dI" % len(words), *words) + packed + q + tags
    return struct.pack("<i", len(body)) + body


# ---- the header ----
def parse_header(text):
    """The ``@`` lines (bytes, every line closed by ``\\n``) -> SamHead(references, lengths, the text as str, the @HD line's SO)."""
    references, lengths, order = [], [], None
    for no, line in enumerate(text.split(b"\n"), 1):
        if line.startswith(b"@SQ\t"):
            kv = dict(p.split(b":", 1) for p in line.split(b"\t")[1:] if b":" in p)
            if b"SN" not in kv or not kv.get(b"LN", b"").isdigit():
                raise SamError("an @SQ line without SN or LN", E_HEADER, no)
            references.append(kv[b"SN"].decode("latin-1"))
            lengths.append(int(kv[b"LN"]))
        elif no == 1 and line.startswith(b"@HD"):
            order = next((p[3:].decode("latin-1") for p in line.split(b"\t")[1:] if p.startswith(b"SO:")), None)
    if not references:
        raise SamError("no @SQ line: a BAM needs its reference dictionary", E_HEADER)
    return SamHead(references, lengths, text.decode("latin-1"), order)


def header_end(path, limit=1 << 30):
    """-> the ``@`` lines' bytes at the start of the file (they end where the first line without ``@`` begins)."""
    out = []
    with open(path, "rb") as f:
        for line in f:
            if line[:1] != b"@":
                break
            out.append(line if line.endswith(b"\n") else line + b"\n")
            limit -= len(line)
            if limit < 0:
                raise SamError("a header of more than 2^30 bytes", E_HEADER)
    return b"".join(out)


def read_sam(path):
    """The whole file on the host -> (SamHead, [every alignment line's BAM record]).  The slow road: tests, and the statement of what
    a file means; errors name their line."""
    header = header_end(path)
    head = parse_header(header)
    tid_of = tid_table(head.references)
    records = []
    with open(path, "rb") as f:
        f.seek(len(header))
        for no, line in enumerate(f, header.count(b"\n") + 1):
            try:
                records.append(encode_line(line[:-1] if line.endswith(b"\n") else line, tid_of))
            except SamError as exc:
                raise exc.at(no) from None
    return head, records


def chunk_places(path, start, chunk_bytes, block=1 << 20):
    """The alignment lines of the file, from byte ``start``, in chunks of at most ``chunk_bytes`` that end behind a newline or with the
    file -> [(file offset, bytes)].  A line longer than ``chunk_bytes`` grows its chunk to the line's end."""
    chunk_bytes = max(int(chunk_bytes), 1)
    places = []
    with open(path, "rb") as f:
        size = f.seek(0, 2)
        at = start
        while at < size:
            want = min(at + chunk_bytes, size)
            end = want
            if want < size:
                f.seek(at)
                end = at + f.read(want - at).rfind(b"\n") + 1     # behind the chunk's last newline; none: at
                while end == at:                                # one line that is longer than the chunk: to its end
                    f.seek(want)
                    more = f.read(block)
                    cut = more.find(b"\n")
                    if cut >= 0:
                        end = want + cut + 1
                    elif not more:
                        end = size
                    want += len(more)
            places.append((at, end - at))
            at = end
    return places


def bam_header_bytes(head):
    """SamHead -> the bytes in front of a BAM's first record: magic, text, reference dictionary."""
    text = head.text.encode("latin-1")
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(head.references))]
    for name, length in zip(head.references, head.lengths):
        n = name.encode("latin-1") + b"\0"
        out += [struct.pack("<i", len(n)), n, struct.pack("<i", length)]
    return b"".join(out)


def tid_table(references):
    return {name.encode("latin-1"): i for i, name in enumerate(references)}


def name_hash(name):
    """FNV-1a, 32 bits: the hash of the device's reference table."""
    h = 0x811C9DC5
    for b in name:
        h = ((h ^ b) * 0x01000193) & 0xFFFFFFFF
    return h


def is_sam_text(start):
    """The first bytes of a file (up to its first line and beyond) -> whether it is SAM text: a first byte ``@``, or a first line of at
    least 11 tab-separated fields."""
    if start[:1] == b"@":
        return True
    if start[:2] == b"\x1f\x8b" or start[:4] == b"BAM\x01" or not start:
        return False
    return start.split(b"\n", 1)[0].count(b"\t") >= 10


# ---- a stream: a pipe, a FIFO, standard input -- text that is seen once ----
STREAM_NAME = "<stdin>"                                         # what ``-`` is called in messages
STREAM_SAM, STREAM_BAM, STREAM_GZIP, STREAM_EMPTY, STREAM_OTHER = "sam", "bam", "gzip", "empty", "other"


def stream_kind(start):
    """The first bytes of a stream -> what it holds: STREAM_SAM (:func:`is_sam_text`), STREAM_BAM (BGZF or gzip magic whose inflated
    head is ``BAM\\1``; a gzip stream that does not inflate counts too: the BAM road names what is broken), STREAM_GZIP (other gzip
    data: compressed SAM), STREAM_EMPTY (no byte), STREAM_OTHER."""
    if not start:
        return STREAM_EMPTY
    if is_sam_text(start):
        return STREAM_SAM
    if start[:2] == b"\x1f\x8b":
        try:
            magic = zlib.decompressobj(31).decompress(bytes(start), 4)
        except zlib.error:
            return STREAM_BAM
        return STREAM_BAM if magic[:4] == b"BAM\x01" else STREAM_GZIP
    return STREAM_OTHER


class StreamReader:
    """A stream of SAM text read ONCE: ``src`` is a file descriptor or an object with ``readinto`` (and, for a descriptor's sake,
    maybe ``fileno``).  :meth:`peek` and :meth:`header` read through a buffer of the reader's own, and what they read beyond what
    they return stays there for :meth:`chunks`.  A descriptor is polled in front of every read, so :meth:`close` ends a reading thread
    within ``POLL_S`` although the writer is silent; ``close`` closes a descriptor the reader owns (``own``), so that the writer ends
    with EPIPE and does not block on a full pipe.  ``wait_pipe`` / ``wait_buffer``: the seconds the thread of :meth:`chunks` waited for
    the stream and for a free buffer; ``text_bytes``: the bytes read so far (of a BAM: its compressed bytes); ``buf_at``: the stream
    offset of the buffer's first byte once :meth:`bam_header` dropped the members in front of the first record's."""
    POLL_S = 0.05
    PEEK = 1 << 16

    def __init__(self, src, own=False):
        self.fd = src if isinstance(src, int) else None
        self.obj = None if isinstance(src, int) else src
        self.own, self.buf, self.eof, self.text_bytes, self.buf_at = own, bytearray(), False, 0, 0
        self.wait_pipe = self.wait_buffer = 0.0
        self._stop, self._thread, self._closed = threading.Event(), None, False
        self._poll = None
        if self.fd is not None:
            self._poll = select.poll()
            self._poll.register(self.fd, select.POLLIN | select.POLLHUP | select.POLLERR)

    # -- one read: up to len(view) bytes into a writable memoryview -> the bytes read, 0 at the end (or when the reader was closed)
    def read_into(self, view):
        if self.fd is None:
            n = self.obj.readinto(view)
            return n or 0
        while not self._stop.is_set():
            if self._poll.poll(int(self.POLL_S * 1000)):
                return os.readv(self.fd, [view])
        return 0

    def _more(self, want=1 << 16):
        """The reader's buffer grown by one read -> whether bytes came."""
        if self.eof:
            return False
        piece = bytearray(want)
        n = self.read_into(memoryview(piece))
        if n <= 0:
            self.eof = True
            return False
        self.buf += piece[:n]
        self.text_bytes += n
        return True

    def peek(self):
        """-> the first bytes of the stream, enough to say what it holds (:func:`stream_kind`): ``PEEK`` bytes of gzip data, else
        the first line (up to 1 MB); they stay in the buffer."""
        while len(self.buf) < 2 and self._more():
            pass
        if self.buf[:2] == b"\x1f\x8b":
            while len(self.buf) < self.PEEK and self._more():
                pass
        else:
            while b"\n" not in self.buf and len(self.buf) < 1 << 20 and self._more():
                pass
        return bytes(self.buf[:1 << 20])

    def header(self, limit=1 << 30):
        """-> the ``@`` lines' bytes, every one closed by ``\\n`` (as :func:`header_end` gives a file's): reading stops behind the first
        line that does not start with ``@``; the bytes read beyond the header stay in the buffer."""
        at = 0
        while True:
            if at == len(self.buf) and not self._more():
                break                                           # the stream ends behind a whole header line
            if self.buf[at] != 64:                              # "@"
                break
            nl, scanned = self.buf.find(b"\n", at), len(self.buf)
            while nl < 0 and self._more():                      # the line goes on: only the bytes that came are searched
                nl, scanned = self.buf.find(b"\n", scanned), len(self.buf)
            if nl < 0:                                          # a last header line without its newline
                self.buf += b"\n"
                nl = len(self.buf) - 1
            at = nl + 1
            if at > limit:
                raise SamError("a header of more than 2^30 bytes", E_HEADER)
        text = bytes(self.buf[:at])
        del self.buf[:at]
        return text

    def chunks(self, range_bytes, first_line=0, alloc=None, buffers=2):
        """The rest of the stream -> (buffer, n_bytes, the number of lines in front of the chunk's first) per chunk: ``buffer[:n_bytes]``
        is about ``range_bytes`` of text cut behind its last newline, the tail carried into the next chunk; a line longer than that
        grows its chunk; a last line without newline is a line.  The chunks cover the stream once, in order, whatever the reads
        return.  ``alloc(n) -> a writable buffer of n bytes`` (default: bytearray; the sort passes pinned memory) is called for
        ``buffers`` (at least two) of them, and again where a long line needs a larger one.  Reading runs on a thread of its own,
        ahead of the caller by the free buffers; a chunk's buffer is the caller's until it asks for the next one."""
        range_bytes = max(int(range_bytes), 1)
        alloc = alloc or bytearray
        free, ready = queue.Queue(), queue.Queue()
        for _ in range(max(int(buffers), 2)):
            free.put(alloc(range_bytes))

        def fill():
            tail, line = bytes(self.buf), first_line
            self.buf = bytearray()
            try:
                while not self._stop.is_set() and (tail or not self.eof):
                    t0 = time.perf_counter()
                    buf = free.get()
                    self.wait_buffer += time.perf_counter() - t0
                    if buf is None:
                        return
                    view = memoryview(buf).cast("B")
                    if len(tail) > len(view):                   # (the header's read-ahead, or a long line's end, beyond a buffer)
                        buf = alloc(2 * len(tail))
                        view = memoryview(buf).cast("B")
                    n = len(tail)
                    view[:n] = tail
                    cut, scanned = _chunk_cut(view, n, range_bytes, self.eof, 0)
                    while not cut and not self.eof:
                        if n == len(view):                      # one line fills the buffer: a larger one
                            bigger = alloc(2 * len(view))
                            memoryview(bigger).cast("B")[:n] = view[:n]
                            buf, view = bigger, memoryview(bigger).cast("B")
                        t0 = time.perf_counter()
                        got = self.read_into(view[n:range_bytes if n < range_bytes else len(view)])
                        self.wait_pipe += time.perf_counter() - t0
                        if got <= 0:
                            self.eof = True
                        else:
                            self.text_bytes += got
                            n += got
                        cut, scanned = _chunk_cut(view, n, range_bytes, self.eof, scanned)
                    if self._stop.is_set():
                        return
                    tail = bytes(view[cut:n])
                    if cut:
                        lines = _count_newlines(view, cut) + (view[cut - 1] != 10)
                        ready.put((buf, cut, line))
                        line += lines
                    else:
                        free.put(buf)
                ready.put(None)
            except BaseException as exc:                        # (handed to the caller, raised there)
                ready.put(exc)

        return self._served(fill, free, ready)

    def _served(self, fill, free, ready):
        """What both chunk generators do with their filling thread: it is started, its chunks are handed on as they get ready -- a
        chunk's buffer goes back to it when the caller asks for the next --, its exception is raised here, and the reader is closed
        when the generator ends or is dropped."""
        self._thread = threading.Thread(target=fill, name="svx-sam-stream", daemon=True)
        self._free = free
        self._thread.start()
        try:
            while True:
                item = ready.get()
                if item is None:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield item
                free.put(item[0])
        finally:
            self.close()

    # -- a BAM on the stream: its header through zlib, then its bytes in chunks of whole BGZF members
    def bam_header(self, limit=1 << 30):
        """The header of a BAM read from the stream: the leading BGZF members inflated with zlib until the text and the reference
        dictionary are complete -> BamStreamHead(``table``: what io.bam.read_bam_header gives for the same bytes as a file; ``first``:
        (the stream offset of the member the first record starts in, the record's offset in that member's inflated bytes, the number
        of references) -- index.first_record's triple; ``head``: the inflated bytes in front of the first record).  The members in
        front of that one are dropped; it and everything read behind it stay in the buffer for :meth:`member_chunks`, and ``buf_at``
        is its stream offset.  A header that fills its members exactly: the first record opens the next one, which need not have
        arrived.  BgzfStreamError: no BGZF member, one that does not inflate, no BAM, a stream that ends inside the header."""
        from .bam import AlignmentTable
        import numpy as np
        head, at, size = bytearray(), 0, _BamHeaderSize()
        while True:
            bsize, xlen = _member_at(self.buf, at, len(self.buf), self.buf_at)
            while not bsize or at + bsize > len(self.buf):
                if not self._more():
                    raise BgzfStreamError("no BGZF block at stream offset %d (the BAM header is cut)" % (self.buf_at + len(self.buf))
                                          if at == len(self.buf) else "no whole BGZF block at stream offset %d" % (self.buf_at + at), self.buf_at + at)
                bsize, xlen = _member_at(self.buf, at, len(self.buf), self.buf_at)
            try:
                data = zlib.decompress(bytes(self.buf[at + 12 + xlen:at + bsize - 8]), -15)
            except zlib.error as exc:
                raise BgzfStreamError("the block at stream offset %d does not inflate (%s)" % (self.buf_at + at, exc), self.buf_at + at) from None
            base = len(head)
            head += data
            need = size(head)
            if need is not None:
                break
            if len(head) > limit:
                raise BgzfStreamError("a BAM header of more than %d bytes" % limit, self.buf_at + at)
            at += bsize
        if need == len(head):                                   # the header fills its member: the first record opens the next one
            at, entry = at + bsize, 0
        else:
            at, entry = at, need - base
        del self.buf[:at]
        self.buf_at += at
        head = bytes(head[:need])
        l_text = struct.unpack_from("<i", head, 4)[0]
        text = head[8:8 + l_text].split(b"\0", 1)[0].decode()   # (the native reader's rule: the text ends at its first NUL)
        n_ref, p = struct.unpack_from("<i", head, 8 + l_text)[0], 12 + l_text
        references, lengths = [], []
        for _ in range(n_ref):
            l_name = struct.unpack_from("<i", head, p)[0]
            references.append(head[p + 4:p + 4 + max(l_name - 1, 0)].decode())
            lengths.append(struct.unpack_from("<i", head, p + 4 + l_name)[0])
            p += 8 + l_name
        none = np.empty(0, np.int32)
        table = AlignmentTable(references, lengths, none, none, none, none, none, none, [], none, np.zeros(1, np.int64), text)
        return BamStreamHead(table, (self.buf_at, entry, n_ref), head)

    def member_chunks(self, range_bytes, alloc=None, buffers=2):
        """The rest of a BGZF stream -> (buffer, n_bytes, the stream offset of the chunk's first byte) per chunk: ``buffer[:n_bytes]``
        is WHOLE BGZF members, found by hopping over the BSIZE fields from the chunk's first byte -- as many as end within
        ``range_bytes``, and at least one; the partial member behind them is carried into the next buffer.  The chunks cover the stream
        once, in order, from what :meth:`peek` and :meth:`bam_header` left in the buffer on, whatever the reads return; none is empty.
        Thread, buffers and :meth:`close` as in :meth:`chunks`; a buffer holds at least one member of the largest size (65,536).
        BgzfStreamError, with the stream offset: a member whose header is not BGZF's (plain gzip has no BC field), a BSIZE too small
        for header and trailer (below 25), a stream that ends inside a member."""
        range_bytes = max(int(range_bytes), 1)
        room = max(range_bytes, MAX_MEMBER)
        alloc = alloc or bytearray
        free, ready = queue.Queue(), queue.Queue()
        for _ in range(max(int(buffers), 2)):
            free.put(alloc(room))

        def fill():
            tail, offset = bytes(self.buf), self.buf_at
            self.buf = bytearray()
            try:
                while not self._stop.is_set() and (tail or not self.eof):
                    t0 = time.perf_counter()
                    buf = free.get()
                    self.wait_buffer += time.perf_counter() - t0
                    if buf is None:
                        return
                    view = memoryview(buf).cast("B")
                    if len(tail) > len(view):                   # (the header's read-ahead beyond a buffer: the larger one takes
                        buf = alloc(len(tail) + MAX_MEMBER)     # its place in the ring for good, so at most ``buffers`` such allocations)
                        view = memoryview(buf).cast("B")
                    n = len(tail)
                    view[:n] = tail
                    cut, at = _member_cut(view, n, range_bytes, self.eof, 0, offset)
                    while not cut and not self.eof:
                        t0 = time.perf_counter()
                        got = self.read_into(view[n:])          # (never full here: a buffer holds the largest member)
                        self.wait_pipe += time.perf_counter() - t0
                        if got <= 0:
                            self.eof = True
                        else:
                            self.text_bytes += got
                            n += got
                        cut, at = _member_cut(view, n, range_bytes, self.eof, at, offset)
                    if self._stop.is_set():
                        return
                    tail = bytes(view[cut:n])
                    if cut:
                        ready.put((buf, cut, offset))
                        offset += cut
                    else:
                        free.put(buf)
                ready.put(None)
            except BaseException as exc:                        # (handed to the caller, raised there)
                ready.put(exc)

        return self._served(fill, free, ready)

    def close(self):
        """The reading thread ended and the descriptor, where the reader owns it, closed; what was not read is dropped."""
        self._stop.set()
        if self._thread is not None:
            self._free.put(None)
            self._thread.join()
            self._thread = None
        if not self._closed:
            self._closed = True
            if self.own and self.fd is not None:
                os.close(self.fd)
            elif self.own and hasattr(self.obj, "close"):
                self.obj.close()


_SEARCH = 1 << 20                                               # bytes of a view copied at a time to be searched


def _find_newline(view, lo, hi, last=False):
    """The first (``last``: the last) newline of view[lo:hi] -> its index, -1: none.  A piece of _SEARCH bytes at a time."""
    starts = range(lo, hi, _SEARCH)
    for at in reversed(starts) if last else starts:
        piece = bytes(view[at:min(at + _SEARCH, hi)])
        k = piece.rfind(b"\n") if last else piece.find(b"\n")
        if k >= 0:
            return at + k
    return -1


def _chunk_cut(view, n, range_bytes, eof, scanned):
    """Where the chunk at the front of view[:n] ends, by the rule of :func:`chunk_places`: behind the last newline of its first
    ``range_bytes``; none there: behind the first one after them (a long line); the stream's end closes the last chunk.  ``scanned``:
    0 for a new chunk, then what the call before returned -- the bytes of the chunk that are known to hold no newline, which are not
    searched again.  -> (the cut, 0: more bytes are needed; ``scanned``)."""
    if n >= range_bytes:
        if scanned < range_bytes:
            at = _find_newline(view, 0, range_bytes, last=True)
            if at >= 0:
                return at + 1, scanned
            scanned = range_bytes
        at = _find_newline(view, scanned, n)
        if at >= 0:
            return at + 1, n
        scanned = n
    return (n if eof else 0), scanned


def _count_newlines(view, n):
    import numpy as np
    return int(np.count_nonzero(np.frombuffer(view[:n], np.uint8) == 10))


# ---- a BGZF stream: its members, hopped over from header to header ----
MAX_MEMBER = 1 << 16                                            # BSIZE is 16 bits: no BGZF member is longer
BamStreamHead = collections.namedtuple("BamStreamHead", "table first head")


class BgzfStreamError(ValueError):
    """A stream that is no chain of whole BGZF members -- ``offset``: the stream offset the message names."""

    def __init__(self, message, offset):
        ValueError.__init__(self, message)
        self.offset = offset


class _BamHeaderSize:
    """``size(head)``, called as the inflated bytes at the start of a BAM grow -> the bytes in front of the first record -- magic, text,
    reference dictionary -- once they are all there, None before.  It goes on where the call before stopped."""

    def __init__(self):
        self.p, self.left = None, None                          # where the next field to read starts, the references still to hop over

    def __call__(self, head):
        if self.p is None:
            if len(head) < 8:
                return None
            if bytes(head[:4]) != b"BAM\x01":
                raise BgzfStreamError("not a BAM: its inflated bytes do not start with the BAM magic", 0)
            l_text = struct.unpack_from("<i", head, 4)[0]
            if l_text < 0:
                raise BgzfStreamError("a malformed BAM header: a text of %d bytes" % l_text, 0)
            self.p = 8 + l_text
        if self.left is None:
            if len(head) < self.p + 4:
                return None
            self.left, self.p = struct.unpack_from("<i", head, self.p)[0], self.p + 4
        while self.left > 0:
            if len(head) < self.p + 4:
                return None
            l_name = struct.unpack_from("<i", head, self.p)[0]
            if l_name < 0:
                raise BgzfStreamError("a malformed BAM header: a reference name of %d bytes" % l_name, 0)
            if len(head) < self.p + 8 + l_name:
                return None
            self.p, self.left = self.p + 8 + l_name, self.left - 1
        return self.p


def _member_at(view, at, n, base=0):
    """The BGZF member whose header starts at view[at], of the n bytes in hand -> (its length by BSIZE, its XLEN); (0, 0): the bytes
    end inside its header.  ``base``: the stream offset of view[0], for the refusal of a header that is not BGZF's -- other magic or
    flags, no BC subfield (plain gzip) -- or whose BSIZE does not hold header and trailer."""
    if n - at < 12:
        if bytes(view[at:min(n, at + 4)]) != b"\x1f\x8b\x08\x04"[:max(n - at, 0)]:
            raise BgzfStreamError("no BGZF block at stream offset %d" % (base + at), base + at)
        return 0, 0
    fixed = bytes(view[at:at + 12])
    if fixed[:3] == b"\x1f\x8b\x08" and not fixed[3] & 4:
        raise BgzfStreamError("no BGZF block at stream offset %d: a gzip member without an extra field (plain gzip is not BGZF)" % (base + at), base + at)
    if fixed[:4] != b"\x1f\x8b\x08\x04":
        raise BgzfStreamError("no BGZF block at stream offset %d" % (base + at), base + at)
    xlen = struct.unpack_from("<H", fixed, 10)[0]
    if n - at < 12 + xlen:
        return 0, 0
    extra, bsize, q = bytes(view[at + 12:at + 12 + xlen]), None, 0
    while q + 4 <= xlen:
        slen = struct.unpack_from("<H", extra, q + 2)[0]
        if extra[q:q + 2] == b"BC" and slen == 2 and q + 6 <= xlen:
            bsize = struct.unpack_from("<H", extra, q + 4)[0] + 1
        q += 4 + slen
    if bsize is None:
        raise BgzfStreamError("no BGZF block at stream offset %d: a gzip member without the BC field (plain gzip is not BGZF)" % (base + at), base + at)
    if bsize < 12 + xlen + 8:
        raise BgzfStreamError("no whole BGZF block at stream offset %d: a BSIZE of %d does not hold its header and trailer" % (base + at, bsize - 1),
                              base + at)
    return bsize, xlen


def _member_cut(view, n, range_bytes, eof, at, base):
    """Where the chunk at the front of view[:n] ends: behind the last member that ends within its first ``range_bytes``; none does:
    behind the first one.  ``at``: 0 for a new chunk, then what the call before returned -- the members up to there are whole and are
    not hopped over again.  -> (the cut, 0: more bytes are needed; ``at``).  The stream's end closes the last chunk, and raises
    BgzfStreamError where it falls inside a member."""
    while True:
        bsize = _member_at(view, at, n, base)[0] if at < n else 0
        if bsize and at + bsize <= n:                           # a whole member
            if at + bsize > range_bytes and at:
                return at, at
            at += bsize
            if at >= range_bytes:
                return at, at
            continue
        if at and n >= range_bytes and at < n:                  # the next member ends behind the bytes in hand, so behind range_bytes
            return at, at
        if eof:
            if at < n:
                raise BgzfStreamError("no whole BGZF block at stream offset %d: the stream ends inside it" % (base + at), base + at)
            return at, at
        return 0, at
