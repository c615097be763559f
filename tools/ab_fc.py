#!/usr/bin/env python3
"""fc6 / fc7 at the CNN batch: svx_fc_bias_act (split count / tile shape forced through an experiment build) vs hipBLASLt.

`ab_fc.py live`: the memo's launch instead -- fc6 + fc7 at M = 256 for live = 8 .. 256, svx_image_dedup at n = 256 and the tail of
the chain (fc7 -> packed rows per record), each captured in a graph of REPS_IN_GRAPH repetitions and replayed 21 times between
HIP events: the median, per repetition.  SVX_TREE=<another built tree> measures that tree's package and library with this tool
(a tree without the fused tail runs fc7 + fc8_softmax + gather_rows there)."""
import os, sys
import torch
sys.path.insert(0, os.environ.get("SVX_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from svision_amd import kernels, _lib
if os.environ.get("SVX_EXP_LIB"):
    _lib.LIB_PATH = os.environ["SVX_EXP_LIB"]
dev = torch.device("cuda:0")
torch.manual_seed(0)


def timed(fn, reps=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


REPS_IN_GRAPH = 10


def graph_us(fn, replays=21):
    """median microseconds of one fn() inside a captured graph of REPS_IN_GRAPH of them"""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        fn()
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            for _ in range(REPS_IN_GRAPH):
                fn()
        g.replay()
        st.synchronize()
        ts = []
        for _ in range(replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            g.replay()
            e1.record(st)
            st.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / REPS_IN_GRAPH)
    return sorted(ts)[len(ts) // 2]


def live_table(m=256):
    x6 = torch.randn(m, 9216, device=dev)
    w6, w7 = (kernels.pack_fc_weights(torch.randn(4096, k, device=dev) / k ** 0.5) for k in (9216, 4096))
    b6, b7, b8 = torch.randn(4096, device=dev), torch.randn(4096, device=dev), torch.randn(5, device=dev)
    w8 = torch.randn(5, 4096, device=dev) / 64
    fused = hasattr(kernels, "fc8_tail")
    print("tree %s  (%s tail), M = %d, microseconds" % (os.environ.get("SVX_TREE") or "own", "fused" if fused else "three-launch", m))
    print("  live | fc6    fc7    fc6+fc7 | fc7 -> packed rows of the records")
    for live in (8, 32, 41, 64, 128, 256):
        lv = torch.tensor([live], dtype=torch.int32, device=dev)
        inv = (torch.arange(m, device=dev, dtype=torch.int32) % live).contiguous()
        x7 = kernels.fc_bias_act(x6, w6, b6, relu=True, live=lv)

        def tail():
            if fused:
                return kernels.fc8_tail(kernels.fc_partial(x7, w7, live=lv), b7, w8, b8, inv, live=lv)
            y = kernels.fc_bias_act(x7, w7, b7, relu=True, live=lv)
            return kernels.gather_rows(kernels.fc8_softmax(y, w8, b8, live=lv), inv)
        t6 = graph_us(lambda: kernels.fc_bias_act(x6, w6, b6, relu=True, live=lv))
        t7 = graph_us(lambda: kernels.fc_bias_act(x7, w7, b7, relu=True, live=lv))
        t67 = graph_us(lambda: kernels.fc_bias_act(kernels.fc_bias_act(x6, w6, b6, relu=True, live=lv), w7, b7, relu=True, live=lv))
        print("  %4d | %6.1f %6.1f %6.1f  | %6.1f" % (live, t6, t7, t67, graph_us(tail)), flush=True)
    from tests.test_image_memo_cpu import planted
    import numpy as np
    recs = planted(seed=21, n=4096)
    for name, r in (("planted duplicates", recs[:256]), ("all equal", np.repeat(recs[:1], 256, axis=0))):
        d = torch.from_numpy(np.ascontiguousarray(r, np.int32)).to(dev)
        live = int(kernels.image_dedup(d)[2].item())
        print("  image_dedup n = 256, %s (live %d): %.1f" % (name, live, graph_us(lambda: kernels.image_dedup(d))), flush=True)


if sys.argv[1:2] == ["live"]:
    live_table()
    sys.exit(0)

for m in (64, 128):
    for name, n, k in (("fc6", 4096, 9216), ("fc7", 4096, 4096)):
        x = torch.randn(m, k, device=dev)
        w = torch.randn(n, k, device=dev) / k ** 0.5
        b = torch.randn(n, device=dev)
        wp = kernels.pack_fc_weights(w)
        ws = torch.empty(64 * 1024 * 1024, device=dev)
        t_lt = timed(lambda: torch._addmm_activation(b, x, w.t(), use_gelu=False))
        row = ["%s m=%d hipBLASLt %.1f us" % (name, m, t_lt)]
        for na in (1, 2):
            for s in [int(v) for v in os.environ.get("SPLITS", "4,8,12,16,21,32").split(",")]:
                os.environ["SVX_FC_SPLITS"], os.environ["SVX_FC_NA"] = str(s), str(na)
                t = timed(lambda: kernels.fc_bias_act(x, wp, b, relu=True, ws=ws))
                row.append("na%d s%d %.1f" % (na, s, t))
        print(" | ".join(row), "  (weights %.0f MB: %.1f us at 6 TB/s)" % (n * k * 4 / 1e6, n * k * 4 / 6e6), flush=True)
