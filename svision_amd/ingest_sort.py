"""A sample from an UNSORTED BAM: its records sorted on the device (``SVX_DEVICE_SORT=1``, svision_amd/cli.py).

An aligner writes its records in the order of the reads; ``samtools sort`` + ``samtools index`` of a 60 GB long-read file take far
longer than the whole run here.  Everything that takes a BAM apart without an index is on the device already (svision_amd/index.py);
what was missing is the order.  :func:`load_sample`:

  pass      the whole file in ranges, the loop of the index build (index.record_ranges): read, inflate, CRC, svx_bam_find_starts,
            svx_bam_walk_count / _extract (``with_seq``: _count_seq / _extract_seq).  Every range's records stay on the device --
            fields, CIGAR words, names, bases --; its inflated and compressed bytes are dropped with the range
  sort      ONE svx_record_sort over all records (csrc/svx_recsort.hip): by (reference, position), records without a reference
            last, ties in file order -- the order `samtools sort` keeps for a file it reads once
  gather    svx_record_gather (tid, pos, flag, mapq, l_seq), svx_record_gather_offsets + svx_record_gather_segments (CIGAR words,
            names, bases) put every array into that order
  table     the arrays the host wants come back through pinned memory, QNAME ids are taken on the SORTED names (svx_name_ids:
            first occurrence in the sorted file), and Sample.from_device scans the gathered CIGARs where they are

The whole file's packed records are resident on the device on this path -- nothing streams out before the last range is read.
The table equals, array for array, read_bam() of the same records written as a file sorted stably by that key.  A corrupt block, a
CRC mismatch, a malformed or cut chain or a device allocation that fails raises SortIngestError; no partial result is returned.
"""
import numpy as np

STAGES = ("read", "upload", "inflate", "crc", "find_starts", "walk", "concat", "sort", "gather", "read_back", "names", "scan")


class SortIngestError(ValueError):
    pass


# ---- planning (host): what svx_record_sort is asked for, and what it does with it ----
def sort_key(tid, pos, n_ref):
    """The key the records are sorted by, ascending (uint64): ((tid < 0 ? n_ref : tid) << 32) | (uint32)(pos + 1)."""
    tid, pos = np.asarray(tid, np.int64), np.asarray(pos, np.int64)
    return (np.where(tid < 0, n_ref, tid).astype(np.uint64) << np.uint64(32)) | (pos + 1).astype(np.uint64)


def pos_bits_for(lengths, max_pos=-1):
    """The significant bits of ``pos + 1``: bit_length(longest reference + 1), at least those of the largest position seen."""
    return max(1, (max([int(v) for v in lengths], default=0) + 1).bit_length(), (int(max_pos) + 1).bit_length())


def digit_plan(n_ref, pos_bits):
    """The passes of the LSD radix sort: the shift of every 8-bit digit of the packed key ((tid') << pos_bits) | (pos + 1), lowest
    first -- pos_bits + bit_length(n_ref) significant bits, at least one pass."""
    bits = int(pos_bits) + int(n_ref).bit_length()
    return [8 * p for p in range(max(1, (bits + 7) // 8))]


def packed_key(tid, pos, n_ref, pos_bits):
    """The key as the kernels pack it (uint64): sort_key with the reference moved down to bit ``pos_bits``."""
    tid, pos = np.asarray(tid, np.int64), np.asarray(pos, np.int64)
    lo = (pos + 1).astype(np.uint64) & np.uint64((1 << int(pos_bits)) - 1)
    return (np.where(tid < 0, n_ref, tid).astype(np.uint64) << np.uint64(pos_bits)) | lo


def _cat(torch, parts, pad, dev):
    """Device arrays end to end, ``pad`` zero elements behind them (what the gathers' aligned loads may touch)."""
    dtype = parts[0].dtype
    return torch.cat(list(parts) + [torch.zeros(pad, dtype=dtype, device=dev)])


def _cat_offsets(torch, parts, totals, dev):
    """Per-range CSR offsets ([n_i + 1] each, from 0) -> one [n + 1] array over the concatenated data."""
    out, at = [], 0
    for off, total in zip(parts, totals):
        out.append(off[:-1] + at)
        at += total
    out.append(torch.full((1,), at, dtype=torch.int64, device=dev))
    return torch.cat(out)


def load_sample(bam_path, fasta, min_sv, device="cuda", with_seq=False, range_bytes=None, stats=None):
    """The :class:`svision_amd.sample.Sample` of a BAM whose records come in any order (see the head of the module).  ``with_seq``: the
    table carries the read bases (--hash / --graph).  ``range_bytes``: compressed bytes a range (default: the device decoder's group
    size; tests).  ``stats``: a dict that receives the number of ranges and records, the CIGAR words and the seconds per stage."""
    from . import index, kernels
    from .io.bam import AlignmentTable, read_bam_header
    from .sample import Sample
    torch, lib, dev, clock = index.on_device("load_sample needs the GPU (svx_record_sort)", device, STAGES)
    try:
        head = read_bam_header(bam_path)
    except ValueError as exc:                                   # (the host reader inflates in front of the header's end: a corrupt block shows here)
        raise SortIngestError(str(exc)) from None
    n_ref = len(head.references)
    fields = ("d_tid", "d_pos", "d_flag", "d_mapq", "d_l_seq")
    parts, n, words, name_bytes, seq_bytes, ranges = [], 0, 0, 0, 0, 0
    try:
        with torch.cuda.device(dev):
            for rng in index.record_ranges(bam_path, head, dev, clock, range_bytes, with_seq=with_seq):
                ranges += 1
                rng.d_raw = rng.d_starts = rng.d_base = None    # the range's inflated bytes go now, not with the next range
                if rng.n_rec:
                    parts.append(rng)
                    n, words, name_bytes, seq_bytes = n + rng.n_rec, words + rng.words, name_bytes + rng.name_bytes, seq_bytes + rng.seq_bytes
            if n > 0xFFFFFFFF:
                raise SortIngestError("%s: %d records -- svx_record_sort takes up to 2^32 - 1" % (bam_path, n))
            if n == 0:
                raise SortIngestError("%s holds no record" % bam_path)
            arrays = _sort_and_gather(torch, kernels, dev, clock, parts, fields, n, words, n_ref, head.lengths, with_seq)
    except index.IndexBuildError as exc:
        raise SortIngestError(str(exc)) from None
    except torch.cuda.OutOfMemoryError as exc:
        raise SortIngestError("%s: the device has no room for the file's packed records -- %d records and %d CIGAR words seen so far (%s)"
                              % (bam_path, n, words, str(exc).split("\n")[0])) from None
    del parts
    host, d_cigar, d_cig_off, d_pos, pos_bits = arrays
    # QNAME ids by first occurrence in the SORTED file (ingest_gpu.DeviceDecoder._make_finish is the pattern)
    names_h = np.ascontiguousarray(host["names"][:name_bytes])
    name_off = np.ascontiguousarray(host["name_off"])
    name_id = np.empty(n, np.int32)
    uniq = np.empty(max(name_bytes, 1), np.uint8)
    ub = np.zeros(1, np.uint64)
    n_unique = int(lib.svx_name_ids(names_h.ctypes.data, name_off.ctypes.data, n, name_id.ctypes.data, uniq.ctypes.data, ub.ctypes.data))
    name_list = uniq[:int(ub[0])].tobytes().decode().split("\n")[:-1] if n_unique else []
    clock.lap("names", False)
    table = AlignmentTable(head.references, head.lengths, host["tid"], host["pos"], host["flag"].view(np.uint16), host["mapq"], host["l_seq"],
                           name_id, name_list, host["cigar"][:words].view(np.uint32), host["cig_off"], head.header_text)
    if with_seq:
        table.seq_packed, table.seq_off = host["seq"][:seq_bytes], host["seq_off"][:n]
    sample = Sample.from_device(table, fasta, min_sv, d_cigar[:max(words, 1)], d_cig_off, d_pos)
    clock.lap("scan")
    if stats is not None:
        stats.update(ranges=ranges, records=n, cigar_words=words, pos_bits=pos_bits, passes=len(digit_plan(n_ref, pos_bits)),
                     seconds={k: round(v, 6) for k, v in clock.times.items()})
    return sample


def _sort_and_gather(torch, kernels, dev, clock, parts, fields, n, words, n_ref, lengths, with_seq):
    """The ranges' arrays end to end, one sort, the gathers, the host's copies -> ({name: host array}, d_cigar with 4 spare words,
    d_cig_off, d_pos, pos_bits), the device arrays in sorted order."""
    cat = {f: torch.cat([getattr(p, f) for p in parts]) for f in fields}
    cat["d_cig_off"] = _cat_offsets(torch, [p.d_cig_off for p in parts], [p.words for p in parts], dev)
    cat["d_name_off"] = _cat_offsets(torch, [p.d_name_off for p in parts], [p.name_bytes for p in parts], dev)
    cat["d_cigar"] = _cat(torch, [p.d_cigar[:p.words] for p in parts], 4, dev)
    cat["d_names"] = _cat(torch, [p.d_names[:p.name_bytes] for p in parts], 4, dev)
    if with_seq:
        cat["d_seq_off"] = _cat_offsets(torch, [p.d_seq_off for p in parts], [p.seq_bytes for p in parts], dev)
        cat["d_seq"] = _cat(torch, [p.d_seq[:p.seq_bytes] for p in parts], 16, dev)
    for p in parts:                                             # the ranges' own arrays go: one copy of the file's records stays
        for f in fields + ("d_cig_off", "d_name_off", "d_cigar", "d_names", "d_seq_off", "d_seq"):
            setattr(p, f, None)
    max_pos = int(cat["d_pos"].max())
    pos_bits = pos_bits_for(lengths, max_pos)
    clock.lap("concat")
    order = kernels.record_sort(cat["d_tid"], cat["d_pos"], n_ref, pos_bits)
    clock.lap("sort")
    out = {f[2:]: kernels.record_gather(cat[f], order) for f in fields}
    segs = [("cigar", "d_cigar", "d_cig_off", "cig_off", 4), ("names", "d_names", "d_name_off", "name_off", 4)]
    if with_seq:
        segs.append(("seq", "d_seq", "d_seq_off", "seq_off", 16))
    for name, data, off, off_name, pad in segs:
        d_off = kernels.record_gather_offsets(cat[off], order)
        total = int(cat[data].numel()) - pad
        d_out = torch.empty(total + pad, dtype=cat[data].dtype, device=dev)
        d_out[total:] = 0                                       # (the scan reads 16-byte quads: 4 readable words behind the CIGARs)
        kernels.record_gather_segments(cat[data], cat[off], order, d_off, d_out)
        out[name], out[off_name] = d_out, d_off
        cat[data] = cat[off] = None
    clock.lap("gather")
    # the host's copies through pinned memory, one event behind them all
    host = {}
    for k, d in out.items():
        h = torch.empty(int(d.numel()), dtype=d.dtype, pin_memory=True)
        h.copy_(d, non_blocking=True)
        host[k] = h
    ev = torch.cuda.Event()
    ev.record()
    ev.synchronize()
    # (copies in ordinary memory: the table outlives this call, and the helper processes of -t N are forked from this one --
    # pinned pages are not mapped into a forked child)
    host = {k: h.numpy().copy() for k, h in host.items()}
    clock.lap("read_back")
    return host, out["cigar"], out["cig_off"], out["pos"], pos_bits
