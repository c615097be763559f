"""Kernel times of the device record sort (svision_amd/csrc/svx_recsort.hip) on synthetic records: svx_record_sort alone, and the sort
plus every gather load_sample makes (five fixed-width arrays, CIGAR words, names).  Device events around the launches, one
warm-up, the median of ``--repeats`` runs; one JSON line per size.  profiles/device_sort.txt holds the protocol and the results.

  python tools/record_sort_bench.py --records 1000000 8000000 --words 300
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    import torch
    from svision_amd import ingest_sort, kernels
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--records", type=int, nargs="+", default=[1_000_000, 8_000_000])
    ap.add_argument("--words", type=int, default=300, help="CIGAR words per record")
    ap.add_argument("--name-bytes", type=int, default=32, help="QNAME bytes per record, the separator included")
    ap.add_argument("--n-ref", type=int, default=3366)
    ap.add_argument("--max-len", type=int, default=248_956_422)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("record_sort_bench needs the GPU: a kernel time cannot be taken anywhere else")
    dev = torch.device("cuda", torch.cuda.current_device())
    pos_bits = ingest_sort.pos_bits_for([args.max_len])
    for n in args.records:
        g = torch.Generator(device=dev)
        g.manual_seed(n)
        d_tid = torch.randint(0, args.n_ref, (n,), generator=g, device=dev, dtype=torch.int32)
        d_pos = torch.randint(0, args.max_len, (n,), generator=g, device=dev, dtype=torch.int32)
        small = {"flag": torch.int16, "mapq": torch.uint8, "l_seq": torch.int32}
        fixed = [d_tid, d_pos] + [torch.zeros(n, dtype=t, device=dev) for t in small.values()]
        d_cig_off = torch.arange(n + 1, device=dev, dtype=torch.int64) * args.words
        d_cigar = torch.randint(0, 1 << 30, (n * args.words + 4,), generator=g, device=dev, dtype=torch.int32)
        d_name_off = torch.arange(n + 1, device=dev, dtype=torch.int64) * args.name_bytes
        d_names = torch.zeros(n * args.name_bytes + 4, dtype=torch.uint8, device=dev)
        d_cigar_out, d_names_out = torch.empty_like(d_cigar), torch.empty_like(d_names)

        def sort_only():
            return kernels.record_sort(d_tid, d_pos, args.n_ref, pos_bits)

        def sort_and_gather():
            order = sort_only()
            for t in fixed:
                kernels.record_gather(t, order)
            for data, off, out in ((d_cigar, d_cig_off, d_cigar_out), (d_names, d_name_off, d_names_out)):
                kernels.record_gather_segments(data, off, order, kernels.record_gather_offsets(off, order), out)
            return order

        def timed(fn):
            fn()                                                # warm-up: code objects, the allocator's blocks
            torch.cuda.synchronize(dev)
            ms = []
            for _ in range(args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            return ms

        sort_ms, all_ms = timed(sort_only), timed(sort_and_gather)
        moved = 2 * (n * args.words * 4 + n * args.name_bytes + n * 15)      # bytes the gathers read + write
        print(json.dumps({"records": n, "cigar_words": args.words, "n_ref": args.n_ref, "pos_bits": pos_bits,
                          "passes": len(ingest_sort.digit_plan(args.n_ref, pos_bits)),
                          "sort_ms": {"median": round(float(np.median(sort_ms)), 3), "all": [round(v, 3) for v in sort_ms]},
                          "sort_and_gathers_ms": {"median": round(float(np.median(all_ms)), 3), "all": [round(v, 3) for v in all_ms]},
                          "gather_bytes": moved,
                          "gather_gb_per_s": round(moved / 1e6 / max(float(np.median(all_ms)) - float(np.median(sort_ms)), 1e-9), 1)}), flush=True)
        del d_cigar, d_cigar_out, d_names, d_names_out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
