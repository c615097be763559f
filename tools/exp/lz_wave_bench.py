"""The three LZ kernels of svx_bgzf_inflate_fast behind their tokens kernels, by launch size: one lane per block (B, svx_lz_core.hpp),
one wave per block (B', round 5) and one workgroup per block (the table kernel, svx_lz_table.hip).  HiFi-like BAM (random bases,
binned qualities), its blocks tiled to the launch sizes.  Per size and kernel: the LZ kernel alone (SVX_INFLATE2_ONLY=B on the
streams an earlier call left in the workspace) and tokens + LZ, HIP events around the launch, median of 7.
python tools/exp/lz_wave_bench.py [contig Mb, default 4] [launch sizes in thousands of blocks, default 7,14,21,28,85]
                                  [kernels, default fast-lane,fast-wave,fast-table] [coverage, default 30] [seed, default 3]
SVX_EXP_LIB: another library than the tree's.  SVX_EXP_WRONG_OUTPUT=1: a measurement-only build of a kernel (SVX_LZT_DBG,
SVX_TOK_DBG), whose bytes are not compared with zlib's."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
import numpy as np
import torch

from svision_amd import _lib, kernels, synth
if os.environ.get("SVX_EXP_LIB"):
    _lib.LIB_PATH = os.environ["SVX_EXP_LIB"]
from svision_amd.io import bam

mb = float(sys.argv[1]) if len(sys.argv) > 1 else 4
t, _g, _ = synth.simulate(synth.SimConfig(contigs=[("c", int(mb * 1e6))], coverage=int(sys.argv[4]) if len(sys.argv) > 4 else 30,
                                          seed=int(sys.argv[5]) if len(sys.argv) > 5 else 3), with_genome=False)
seg = bam.encode_reference_segment(t, seq="random", seed=1)
path = "/tmp/lzw_%d.bam" % os.getpid()
bam.write_bam_segments(path, t.references, t.lengths, [seg])
raw = np.fromfile(path, np.uint8)
os.unlink(path)
src_off, src_len, isize, _b = kernels.bgzf_block_table(raw)
padded = np.zeros((raw.size + 31) // 16 * 16, np.uint8)
padded[:raw.size] = raw
d = torch.from_numpy(padded).cuda()
want = bam.bgzf_decompress(raw.tobytes())
n0 = len(isize)
print("%d blocks, %.1f MB inflated" % (n0, len(want) / 1e6), flush=True)
lib = _lib.load()


def run(variant, k, only=None):
    s, l, z = (np.concatenate([a] * k) for a in (src_off, src_len, isize))
    if only:
        os.environ["SVX_INFLATE2_ONLY"] = only
    best = 1e9
    out = None
    try:
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, status = kernels.bgzf_inflate(d, s, l, z, wave=variant, crc=False)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
    finally:
        os.environ.pop("SVX_INFLATE2_ONLY", None)
    return best, out, status


VARIANTS = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else ("fast-lane", "fast-wave", "fast-table")
WRONG_OUTPUT = os.environ.get("SVX_EXP_WRONG_OUTPUT") == "1"
for variant in VARIANTS:
    _t, out, status = run(variant, 1)
    ok = not bool(status.any()) and (WRONG_OUTPUT or out.cpu().numpy().tobytes() == want)
    print(variant, "== zlib:", ok, flush=True)
    assert ok


def events_ms(variant, k, only=None, reps=7):
    """One launch of ``k`` copies of the file's blocks, everything uploaded and allocated beforehand -> median milliseconds."""
    s, l, z = (np.concatenate([a] * k) for a in (src_off, src_len, isize))
    n = len(z)
    dst = np.zeros(n + 1, np.uint64)
    dst[1:] = np.cumsum(z.astype(np.uint64))
    total = int(dst[-1])
    dev = d.device
    d_src, d_len = torch.from_numpy(s.view(np.int64)).to(dev), torch.from_numpy(l.view(np.int32)).to(dev)
    d_dst = torch.from_numpy(dst.view(np.int64)).to(dev)
    d_out = torch.empty(total, dtype=torch.uint8, device=dev)
    d_status = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = kernels.inflate_workspace(lib, "fast", total, n, dev)

    def launch():
        kernels.launch_inflate(lib, variant, d.data_ptr(), d_src.data_ptr(), d_len.data_ptr(), d_dst.data_ptr(), n, d_out.data_ptr(),
                               d_status.data_ptr(), total, dev, ws=ws)
    launch()                                                  # (leaves the streams in the workspace for the LZ-only runs)
    torch.cuda.synchronize()
    assert not bool(d_status.any())
    times = []
    if only:
        os.environ["SVX_INFLATE2_ONLY"] = only
    try:
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
    finally:
        os.environ.pop("SVX_INFLATE2_ONLY", None)
    return float(np.median(times)), n


sizes = [int(float(v) * 1000) for v in (sys.argv[2] if len(sys.argv) > 2 else "7,14,21,28,85").split(",")]
print("blocks   " + "   ".join("%-34s" % (v + ": LZ alone | tokens + LZ (ms)") for v in VARIANTS), flush=True)
for size in sizes:
    k = max(1, round(size / n0))
    row = []
    for variant in VARIANTS:
        lz_ms, n = events_ms(variant, k, only="B")
        all_ms, n = events_ms(variant, k)
        row.append("%-34s" % ("%7.2f | %7.2f" % (lz_ms, all_ms)))
    print("%6d   " % n + "   ".join(row), flush=True)
