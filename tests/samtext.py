"""Record dicts -> SAM text, and the dicts tests/htslike.encode_record is handed for the same records.  Test-side: a reading of SAMv1
section 1.4 / 1.5 of its own that shares no code with svision_amd/io/sam.py.

A record is htslike's dict (tid, pos, qname, flag, mapq, cigar=[(n, op)], seq, qual=bytes of phred values or None, tags, next_tid,
next_pos, tlen) with two liberties that only the text can express: a tag of type ``"i"`` carries a Python int whose BAM type the
reader chooses, and a tag of type ``"f"`` / ``"Bf"`` carries its decimal TEXT (a str / a list of str)."""

_B_JOIN = ","


def narrowed(value):
    """The BAM type htslib gives a SAM ``i`` value: the smallest that holds it, signed only where the value is negative."""
    if value < 0:
        for typ, lowest in (("c", -2 ** 7), ("s", -2 ** 15), ("i", -2 ** 31)):
            if value >= lowest:
                return typ
    else:
        for typ, highest in (("C", 2 ** 8), ("S", 2 ** 16), ("I", 2 ** 32)):
            if value < highest:
                return typ
    raise ValueError("no BAM integer type holds %d" % value)


def for_htslike(rec):
    """The dict for htslike.encode_record: ``i`` tags narrowed, ``f`` texts as the float nearest to the decimal, bases as stored."""
    tags = []
    for name, typ, value in rec.get("tags", []):
        if typ == "i":
            typ = narrowed(value)
        elif typ == "f":
            value = float(value)
        elif typ == "Bf":
            value = [float(v) for v in value]
        tags.append((name, typ, value))
    seq = rec.get("seq", "*")
    if seq != "*":                                              # the base a reader stores: either case, what the table lacks is N
        seq = "".join(c.upper() if c.upper() in "=ACMGRSVTWYHKDBN" else "N" for c in seq)
    return dict(rec, tags=tags, seq=seq)


def _tag_text(name, typ, value):
    if typ in "AZH":
        return "%s:%s:%s" % (name, typ, value)
    if typ == "i":
        return "%s:i:%d" % (name, value)
    if typ == "f":
        return "%s:f:%s" % (name, value)
    assert typ[0] == "B" and len(typ) == 2, typ
    return "%s:B:%s" % (name, _B_JOIN.join([typ[1]] + [str(v) for v in value]))


def line(rec, references):
    """One record -> its SAM line (bytes, no newline).  ``references``: [(name, length)]."""
    def ref(tid):
        return "*" if tid < 0 else references[tid][0]
    next_tid = rec.get("next_tid", -1)
    seq = rec.get("seq", "*")
    qual = rec.get("qual")
    cols = [rec["qname"], str(rec["flag"]), ref(rec["tid"]), str(rec["pos"] + 1), str(rec["mapq"]),
            "".join("%d%s" % c for c in rec.get("cigar", [])) or "*",
            "=" if next_tid >= 0 and next_tid == rec["tid"] else ref(next_tid), str(rec.get("next_pos", -1) + 1), str(rec.get("tlen", 0)),
            seq, "*" if qual is None else "".join(chr(q + 33) for q in qual)]
    cols += [_tag_text(*t) for t in rec.get("tags", [])]
    return "\t".join(cols).encode("latin-1")


def header_text(references, hd="@HD\tVN:1.6\tSO:unsorted\n", extra="@PG\tID:aligner\tPN:aligner\n"):
    return hd + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in references) + extra


def text(references, records, header=None, last_newline=True):
    """A whole file: header + one line a record."""
    body = b"\n".join(line(r, references) for r in records)
    if records and last_newline:
        body += b"\n"
    return (header_text(references) if header is None else header).encode("latin-1") + body


def records_of_table(table, rng=None, tags=False):
    """An AlignmentTable (svision_amd.io.bam.read_bam, svision_amd.synth.simulate; with or without read bases) -> record dicts in the
    table's order.  ``rng`` (numpy Generator): phred values for the reads that carry bases; ``tags``: NM:i, an rq:f of four decimals,
    and on every 16th read an MM:Z / ML:B:C pair."""
    import numpy as np
    ops = "MIDNSHP=X"
    letters = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)
    packed = None if table.seq_packed is None else np.frombuffer(bytes(table.seq_packed), np.uint8)
    out = []
    for i in range(len(table.tid)):
        words = table.cigar[int(table.cig_off[i]):int(table.cig_off[i + 1])]
        rec = dict(qname=table.names[int(table.name_id[i])], tid=int(table.tid[i]), pos=int(table.pos[i]), flag=int(table.flag[i]),
                   mapq=int(table.mapq[i]), cigar=[(int(w) >> 4, ops[int(w) & 15]) for w in words], seq="*", qual=None, tags=[])
        n = int(table.l_seq[i])
        if packed is not None and n:
            at = int(table.seq_off[i])
            end = int(table.seq_off[i + 1]) if i + 1 < len(table.seq_off) else packed.size
            if end - at >= (n + 1) // 2:                        # (a table may count bases of a read whose record carries none)
                raw = packed[at:at + (n + 1) // 2]
                codes = np.empty(2 * raw.size, np.uint8)
                codes[0::2], codes[1::2] = raw >> 4, raw & 15
                rec["seq"] = letters[codes[:n]].tobytes().decode()
                if rng is not None:
                    rec["qual"] = bytes(rng.integers(0, 94, n, dtype=np.uint8))
        if tags:
            rec["tags"] = [("NM", "i", int(i * 37 % 70000) - 200), ("rq", "f", "0.%04d" % (i * 7919 % 10000))]
            if i % 16 == 0 and rng is not None:
                k = int(rng.integers(1, 600))
                rec["tags"] += [("MM", "Z", "C+m?" + "".join(",%d" % v for v in rng.integers(0, 30, k)) + ";"),
                                ("ML", "BC", [int(v) for v in rng.integers(0, 256, k)])]
        out.append(rec)
    return out
