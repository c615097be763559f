"""The header of a sorted BAM, and the one header of several inputs (host, NumPy only): what svision_amd/sort.py writes in front of
the records and what svision_amd/ingest_sort.py numbers the references of several inputs by.

  header    the input's header with its @HD line set to SO:coordinate (VN kept, GO and SS dropped; no @HD: one is prepended; nothing
            else is added, no @PG line: the output is reproducible byte for byte), in blocks of its own through the same encoder; the
            first record opens a new block.  The encoder's member of an empty block is the 28-byte end-of-file marker, which closes
            the file
"""
import collections
import struct

import numpy as np


class SortWriteError(ValueError):
    pass


def sorted_header_text(text):
    """The header text with its @HD line saying ``SO:coordinate``: VN kept (1.6 where there is none), GO and SS -- they describe the
    old order -- dropped, every other field and every other line as it is; without an @HD line one is prepended."""
    lines = text.split("\n")
    if lines and lines[0].startswith("@HD"):
        fields = lines[0].split("\t")[1:]
        vn = next((f for f in fields if f.startswith("VN:")), "VN:1.6")
        rest = [f for f in fields if f[:3] not in ("VN:", "SO:", "GO:", "SS:")]
        lines[0] = "\t".join(["@HD", vn, "SO:coordinate"] + rest)
        return "\n".join(lines)
    return "@HD\tVN:1.6\tSO:coordinate\n" + text


# ``renames``: per input the table its records need under ``retag``, {("RG", old ID): new ID, ("PG", old ID): new ID} with the IDs as
# bytes -- empty for most inputs, and for all of them without ``retag``.
MergedHeader = collections.namedtuple("MergedHeader", "text references lengths maps renames", defaults=((),))


def _line_fields(line):
    """A header line's TAG:VALUE fields -> {tag: value} (the first of a tag counts)."""
    out = {}
    for f in line.split("\t")[1:]:
        if len(f) > 2 and f[2] == ":":
            out.setdefault(f[:2], f[3:])
    return out


def _with_fields(line, new):
    """The line with the value of every field in ``new`` {tag: value} replaced, everything else as it is."""
    return "\t".join(f[:3] + new[f[:2]] if i and len(f) > 2 and f[2] == ":" and f[:2] in new else f for i, f in enumerate(line.split("\t")))


def merge_headers(parts, retag=False):
    """The headers of several inputs -> MergedHeader(the merged text, through :func:`sorted_header_text`; the merged references and
    lengths; per input an int32 table ``map[old refID] -> merged refID``).  ``parts``: per input (its name for messages, the header
    text, its references, their lengths) -- the dictionary a BAM carries in binary, a SAM in its @SQ lines; a headerless SAM part has
    neither.  One input: its text through sorted_header_text and nothing else.  The rules:

      @HD   the first input's (sorted_header_text: SO:coordinate; none: one is prepended); a later input's is dropped
      @SQ   the union by SN in order of first appearance, the inputs taken in list order; the first occurrence's whole line is kept
            (a reference a BAM's text has no line for gets ``@SQ SN LN``); the same SN with another LN: SortWriteError
      @RG   the union by ID, an identical line once; the same ID on another line: SortWriteError (the records' RG:Z tags would have
            to be rewritten).  Under ``retag`` they are: the later input's line is renamed ID-<1-based input number>, the rule of
            @PG; the first input to bring an ID keeps it; a new name that is itself taken -- by an earlier input or by a line of
            the input's own -- is refused
      @PG   the union by ID, an identical line once; the same ID on another line: the later input's line is renamed ID-<1-based input
            number>, and the PP fields of that input's other @PG lines follow.  The records' PG:Z tags are NOT rewritten, unless
            under ``retag``
    ``retag``: the result's ``renames`` holds per input what its records need, {("RG", old): new, ("PG", old): new} as bytes (the
    caller rewrites the records' RG:Z / PG:Z values: svx_record_retag_measure / svx_record_retag_write); unset, every table is empty
    and a renamed @PG line is a change of the header alone.
      other lines (@CO, ...): in input order, a line that is already there once
    A later input's new line goes behind the last line of its type so far (no such line: to the end), so the types stay together."""
    parts = [(name, text, list(refs), [int(v) for v in lens]) for name, text, refs, lens in parts]
    if len(parts) == 1:
        _name, text, refs, lens = parts[0]
        return MergedHeader(sorted_header_text(text), refs, lens, [np.arange(len(refs), dtype=np.int32)], [{}])
    out, seen, sq_seen = [], set(), set()                       # the merged lines, the lines that are there, the SN that have a line
    tid_of, owner, references, lengths, maps, renames = {}, {}, [], [], [], []
    rg, pg = {}, {}                                             # ID -> (line, input's name)

    def add(line):
        at = next((i + 1 for i in range(len(out) - 1, -1, -1) if out[i][:3] == line[:3]), len(out))
        out.insert(at, line)
        seen.add(line)

    for k, (name, text, refs, lens) in enumerate(parts, 1):
        lines = [l for l in text.split("\n") if l.strip("\0")]
        # ---- the dictionary: the union by name, and this input's table
        table = np.empty(len(refs), np.int32)
        for i, (ref, n) in enumerate(zip(refs, lens)):
            if ref not in tid_of:
                tid_of[ref], owner[ref] = len(references), name
                references.append(ref)
                lengths.append(n)
            elif lengths[tid_of[ref]] != n:
                raise SortWriteError("%s and %s name the reference %s with different lengths: %d and %d -- they were not aligned to the "
                                     "same reference" % (owner[ref], name, ref, lengths[tid_of[ref]], n))
            table[i] = tid_of[ref]
        maps.append(table)
        # ---- @PG: which IDs of this input take the suffix (a rename changes the PP of other lines, which may rename those too)
        renamed = {}
        while k > 1:
            before = len(renamed)
            for l in lines:
                f = _line_fields(l) if l.startswith("@PG\t") else {}
                new = _with_fields(l, {"PP": renamed[f["PP"]]}) if f.get("PP") in renamed else l
                if f.get("ID") in pg and pg[f["ID"]][0] != new:
                    renamed[f["ID"]] = "%s-%d" % (f["ID"], k)
            if len(renamed) == before:
                break
        # ---- the lines: the first input's as they are, a later input's where they are new -- its new references first, in the
        # dictionary's order, then the rest in the text's
        sq_line = {}
        for l in lines:
            if l.startswith("@SQ\t"):
                sq_line.setdefault(_line_fields(l).get("SN"), l)

        def add_sq():
            for ref in refs:
                if ref not in sq_seen:
                    add(sq_line.get(ref) or "@SQ\tSN:%s\tLN:%d" % (ref, lengths[tid_of[ref]]))
                    sq_seen.add(ref)
        if k > 1:
            add_sq()
        own_rg = {_line_fields(l).get("ID") for l in lines if l.startswith("@RG\t")}
        rg_renamed = {}
        for i, l in enumerate(lines):
            kind, f = l[:3], _line_fields(l)
            if kind == "@HD":
                if k == 1 and i == 0:
                    out.append(l)
                continue
            if kind == "@SQ":
                if k > 1:
                    continue
                sq_seen.add(f.get("SN"))
            if kind == "@RG" and "ID" in f:
                new_id = f["ID"]
                if k > 1 and f["ID"] in rg and rg[f["ID"]][0] != l:
                    if not retag:
                        raise SortWriteError("%s and %s both have a read group %s, on different @RG lines -- one of them would need its records' "
                                             "RG:Z tags rewritten, which this tool does not do: give the read groups distinct IDs.  Under "
                                             "retag (--retag, SVX_SORT_RETAG=1; sort_bam's retag) the later one is renamed and its BAM "
                                             "records follow" % (rg[f["ID"]][1], name, f["ID"]))
                    new_id = "%s-%d" % (f["ID"], k)
                    if new_id in rg or new_id in own_rg:
                        raise SortWriteError("%s and %s both have a read group %s, on different @RG lines, and the name %s that the later one "
                                             "would take is in use too (%s): give the read groups distinct IDs"
                                             % (rg[f["ID"]][1], name, f["ID"], new_id, rg[new_id][1] if new_id in rg else name))
                    rg_renamed[f["ID"]] = new_id
                    l = _with_fields(l, {"ID": new_id})
                rg.setdefault(new_id, (l, name))
            if kind == "@PG" and "ID" in f:
                change = {t: renamed[f[t]] for t in ("ID", "PP") if f.get(t) in renamed}
                l = _with_fields(l, change) if change else l
                pg.setdefault(renamed.get(f["ID"], f["ID"]), (l, name))
            if k == 1:
                out.append(l)
                seen.add(l)
            elif l not in seen:
                add(l)
        add_sq()                                                # (the first input's dictionary entries that its text has no line for)
        renames.append({(tag, old.encode("latin-1")): new.encode("latin-1") for tag, table in (("RG", rg_renamed), ("PG", renamed))
                        for old, new in table.items()} if retag else {})
    if not references:
        raise SortWriteError("%s: no input has an @SQ line: a BAM needs its reference dictionary" % parts[0][0])
    return MergedHeader(sorted_header_text("\n".join(out) + "\n"), references, lengths, maps, renames)


def sorted_header_bytes(head):
    """The inflated bytes in front of a BAM's first record -> the same with the text rewritten by :func:`sorted_header_text`; the
    reference dictionary behind the text is kept byte for byte."""
    if head[:4] != b"BAM\x01":
        raise SortWriteError("not a BAM header")
    l_text = struct.unpack_from("<i", head, 4)[0]
    text = head[8:8 + l_text].rstrip(b"\0").decode("latin-1")
    new = sorted_header_text(text).encode("latin-1")
    return b"BAM\x01" + struct.pack("<i", len(new)) + new + head[8 + l_text:]
