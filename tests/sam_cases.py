"""The ONE case list of the SAM tests (tests/test_sam_cpu.py, tests/test_gpu_sam_parse.py, tests/test_gpu_sort_sam.py): the smallest
shapes at which a SAM line can be parsed wrongly.  Records are tests/samtext.py's dicts; ``cases()`` -> [(name, record, refused)],
``refused``: the kernels hand the line to the host (SVX_SAM_HOST) -- the 65,536-operation CIGAR and the five ``f`` spellings outside
the exact fast path, and nothing else.  ``errors()`` -> [(name, text of a whole file, the 1-based number of the bad line or None for
the header, the kernels' code or None where the header is what is wrong)]."""
import functools
import random

from tests import samtext

N_REFS = 3366
REFS = [("ref%04d" % i if i else "chr1", 1 << 29) for i in range(N_REFS - 1)] + [("the_last|reference:1-2", 12345)]
SEQ_LENGTHS = ("*", 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 70000)
I_VALUES = (-2 ** 31, -32769, -32768, -129, -128, -1, 0, 255, 256, 65535, 65536, 2 ** 32 - 1)
F_FAST = ("0", "-0", "1", "0.1", "0.3", "0.0123", "1e-5", "123456789012345e7")
F_REFUSED = ("1234567890123456789", "1e30", "1e-30", "inf", "nan")
# a span across the edge of each of the five reg2bin levels: (pos, reference bases), the edge at a multiple of 2^14 .. 2^26
BIN_EDGES = tuple(((1 << s) * 3 - 5, 10) for s in (14, 17, 20, 23, 26)) + (((1 << 14) - 1, 1), (1 << 14, 1), ((1 << 26) - 3, 1 << 27))


def _rec(name, tid=0, pos=1000, flag=0, mapq=60, cigar=(), seq="*", qual=None, tags=(), **more):
    return dict(qname=name, tid=tid, pos=pos, flag=flag, mapq=mapq, cigar=list(cigar), seq=seq, qual=qual, tags=list(tags), **more)


def _read(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def random_decimals(rng, n):
    """Decimal texts inside the fast path: 1 to 15 digits, a point anywhere, an exponent that keeps the decimal exponent within 22."""
    out = []
    for _ in range(n):
        digits = "".join(rng.choice("0123456789") for _ in range(rng.randint(1, 15)))
        cut = rng.randint(0, len(digits))
        t = digits[:cut] + ("." + digits[cut:] if cut < len(digits) or rng.random() < 0.2 else "")
        if t.startswith("."):
            t = rng.choice(("0", "")) + t
        if rng.random() < 0.5:
            t += rng.choice("eE") + rng.choice(("", "+", "-")) + str(rng.randint(0, 7))
        out.append(rng.choice(("", "", "-", "+")) + t)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    rng = random.Random(20)
    out = []

    def add(name, refused=False, **kw):
        out.append((name, _rec(name, **kw), refused))
    # ---- line shape
    for n in SEQ_LENGTHS:
        if n == "*":
            add("seq_star")
            continue
        add("seq_%d" % n, pos=5000 + n, cigar=[(n, "M")], seq=_read(rng, n), qual=bytes(rng.randrange(0, 94) for _ in range(n)))
    add("seq_lower", cigar=[(8, "M")], seq="acgtnACG", qual=bytes(range(8)))
    add("seq_iupac", cigar=[(16, "=")], seq="=ACMGRSVTWYHKDBN", qual=bytes(range(16)))
    add("seq_iupac_lower_odd", cigar=[(15, "X")], seq="acmgrsvtwyhkdbn")
    add("seq_question_mark", cigar=[(5, "M")], seq="AC?T.", qual=bytes(5))
    add("qual_star", cigar=[(5, "M")], seq="ACGTA")
    add("qual_lowest", cigar=[(5, "M")], seq="ACGTA", qual=bytes([0] * 5))
    add("qual_highest", cigar=[(5, "M")], seq="ACGTA", qual=bytes([93] * 5))
    # ---- core fields
    for flag in (0, 4, 2064, 65535):
        add("flag_%d" % flag, flag=flag)
    add("mapq_0", mapq=0)
    add("mapq_255", mapq=255)
    add("pos_0", tid=-1, pos=-1, flag=4)
    add("pos_max", tid=-1, pos=2 ** 31 - 2, flag=4)
    add("tlen_max", tlen=2 ** 31 - 1, next_tid=0, next_pos=77)
    add("tlen_min", tlen=-(2 ** 31 - 1), next_tid=0, next_pos=2 ** 31 - 2)
    add("rname_first", tid=0)
    add("rname_last", tid=N_REFS - 1, pos=3)
    add("rnext_same", tid=7, next_tid=7, next_pos=10)
    add("rnext_none", tid=7, next_tid=-1)
    add("rnext_other", tid=7, next_tid=N_REFS - 1, next_pos=1)
    add("rnext_of_unplaced", tid=-1, pos=-1, flag=4, next_tid=3, next_pos=9)
    add("unmapped_with_reference", tid=5, pos=123456, flag=4)
    add("unmapped_without", tid=-1, pos=-1, flag=4, seq="ACGT", qual=bytes(4))
    for k, (pos, span) in enumerate(BIN_EDGES):
        add("bin_edge_%d" % k, tid=1, pos=pos, cigar=[(span, "M")])
    # ---- CIGAR
    add("cigar_one", cigar=[(1, "M")])
    for n in (63, 64, 65):
        add("cigar_%d_ops" % n, cigar=[(rng.randint(1, 30), "MID"[i % 3]) for i in range(n)])
    add("cigar_digits", cigar=[(int("123456789"[:d]), "M") for d in range(1, 9)] + [(2 ** 28 - 1, "D"), (10 ** 8, "N")], tid=2, pos=0)
    add("cigar_letters", cigar=[(3, "H"), (4, "S"), (5, "M"), (6, "I"), (7, "D"), (8, "N"), (9, "P"), (10, "="), (11, "X"), (2, "S")])
    many = [(1 + i % 3, "MI"[i & 1]) for i in range(65536)]
    add("cigar_65535_ops", cigar=many[:65535], tid=3, pos=100)
    add("cigar_65536_ops", refused=True, cigar=many, tid=3, pos=200, tags=[("NM", "i", 3)])
    # ---- tags
    add("tag_none")
    add("tag_A", tags=[("XA", "A", "q"), ("XB", "A", ":")])
    add("tag_Z", tags=[("Z0", "Z", ""), ("Z1", "Z", "with spaces  in it "), ("Z2", "Z", "a:b::c:"), ("Z3", "Z", "x" * 200)])
    add("tag_H", tags=[("XH", "H", "1AE301"), ("YH", "H", "")])
    add("tag_i", tags=[("I%X" % k, "i", v) for k, v in enumerate(I_VALUES)])
    add("tag_B", tags=[("Bc", "Bc", [-128, 0, 127]), ("BC", "BC", [0, 255]), ("Bs", "Bs", [-32768, 32767, -1]), ("BS", "BS", [65535, 0, 7, 9]),
                       ("Bi", "Bi", [-2 ** 31, 2 ** 31 - 1]), ("BI", "BI", [2 ** 32 - 1, 0]), ("Bf", "Bf", ["1.5", "-2", "3e2"]), ("B0", "Bc", [])])
    add("tag_B_longer_than_a_step", tags=[("BS", "BS", list(range(990, 1090)))])
    add("tag_ML_MM", cigar=[(50, "M")], seq=_read(rng, 50), qual=bytes(50),
        tags=[("MM", "Z", "C+m?" + "".join(",%d" % rng.randint(0, 40) for _ in range(2400)) + ";"), ("ML", "BC", [rng.randrange(256) for _ in range(5000)])])
    add("tag_f", tags=[("F%d" % k, "f", v) for k, v in enumerate(F_FAST)])
    add("tag_Bf_10000", tags=[("XF", "Bf", random_decimals(rng, 10000)), ("XZ", "Z", "behind the array")])
    for k, v in enumerate(F_REFUSED):
        add("tag_f_refused_%d" % k, refused=True, tags=[("XF", "f", v)] if k != 1 else [("XG", "Bf", ["1", v, "2"])])
    return out


def records():
    return [rec for _name, rec, _refused in cases()]


def refused_lines():
    """The 0-based indices, among the cases, of the lines the kernels hand back."""
    return [i for i, (_name, _rec_, refused) in enumerate(cases()) if refused]


def case_text(last_newline=True):
    """-> (the whole file's text, the byte offset of its first alignment line)."""
    head = samtext.header_text(REFS).encode()
    return samtext.text(REFS, records(), last_newline=last_newline), len(head)


# codes of include/svx.h (SVX_SAM_E_*), written out: the tests do not take them from the product
E_FIELDS, E_NUMBER, E_NAME, E_RNAME, E_CIGAR, E_QUAL, E_TAG, E_RANGE, E_HEADER = -2, -3, -4, -5, -6, -7, -8, -9, -10


def errors():
    good = [samtext.line(_rec("good%d" % k, pos=100 * k, cigar=[(4, "M")], seq="ACGT", qual=bytes(4)), REFS) for k in range(3)]
    head = samtext.header_text(REFS).encode()
    n_head = head.count(b"\n")

    def broken(line_):
        return head + b"\n".join([good[0], good[1], line_, good[2]]) + b"\n", n_head + 3

    def edit(col, value, rec=None):
        cols = (samtext.line(rec, REFS) if rec else good[1]).split(b"\t")
        cols[col] = value
        return b"\t".join(cols)
    tagged = _rec("t", tags=[("XI", "i", 0)])
    out = [("empty_line",) + broken(b"") + (E_FIELDS,),
           ("ten_fields",) + broken(b"\t".join(good[1].split(b"\t")[:10])) + (E_FIELDS,),
           ("pos_12x",) + broken(edit(3, b"12x")) + (E_NUMBER,),
           ("qual_short",) + broken(edit(10, b"III")) + (E_QUAL,),
           ("unknown_rname",) + broken(edit(2, b"chrUnknown")) + (E_RNAME,),
           ("i_2_32",) + broken(edit(11, b"XI:i:4294967296", tagged)) + (E_RANGE,),
           ("name_255",) + broken(edit(0, b"n" * 255)) + (E_NAME,),
           ("header_behind_record",) + broken(b"@CO\tlate") + (E_HEADER,),
           ("no_sq", b"@HD\tVN:1.6\n@PG\tID:x\n" + b"\n".join(good) + b"\n", None, None)]
    return out
