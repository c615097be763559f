"""Device ops of the hot path: thin wrappers that hand torch-owned device
buffers to the C ABI of libsvx.so on the current HIP stream.

PyTorch is used here only for device memory and streams.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

GAP_DTYPE = np.dtype([("aln", "<u4"), ("op", "<u4"), ("read_pos", "<i4"),
                      ("ref_pos", "<i4"), ("len", "<i4"), ("kind", "<u4")])
MEAN = (104.0, 117.0, 124.0)   # reference src/network/create_batch.py:13


# ---- layout plumbing (torch ops, once per model / in tests; include/svx.h describes the layouts) ----
def to_c8(x):
    """NCHW [n,C,H,W] -> C8 [n,C/8,H,W,8] (contiguous)."""
    n, c, h, w = x.shape
    if c % 8:
        raise _lib.SvxError("the C8 layout needs a channel count that is a multiple of 8")
    return x.reshape(n, c // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous()


def from_c8(x):
    """C8 [n,C/8,H,W,8] -> NCHW [n,C,H,W] (contiguous)."""
    n, o, h, w, e = x.shape
    return x.permute(0, 1, 4, 2, 3).reshape(n, o * e, h, w).contiguous()


def pack_conv_weights(w_hwio):
    """Checkpoint conv weights HWIO [k,k,cin_g,cout] -> [k,k,cin_g/8,cout,8] (svx_conv2d_same's d_w_packed)."""
    k, k2, cin_g, cout = w_hwio.shape
    if cin_g % 8:
        raise _lib.SvxError("cin/groups must be a multiple of 8")
    return w_hwio.reshape(k, k2, cin_g // 8, 8, cout).permute(0, 1, 2, 4, 3).contiguous()


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_cuda(t, name):
    if not t.is_cuda:
        raise _lib.SvxError(f"{name} must be a device tensor (got {t.device}); the hot path has no CPU fallback")
    if not t.is_contiguous():
        raise _lib.SvxError(f"{name} must be contiguous")


def rasterize(records, layout="NCHW", mean=MEAN, out=None):
    """records: int32 device tensor [n,12] -> float32 [n,3,227,227] (NCHW) or
    [n,227,227,3] (NHWC), mean-subtracted.  See include/svx.h svx_rasterize."""
    lib = _lib.load()
    _require_cuda(records, "records")
    if records.dtype != torch.int32 or records.dim() != 2 or records.shape[1] != 12:
        raise _lib.SvxError("records must be int32 [n,12]")
    n = records.shape[0]
    lay = {"NHWC": _lib.LAYOUT_NHWC, "NCHW": _lib.LAYOUT_NCHW}[layout]
    shape = (n, _lib.IMG, _lib.IMG, 3) if lay == _lib.LAYOUT_NHWC else (n, 3, _lib.IMG, _lib.IMG)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=records.device)
    else:
        _require_cuda(out, "out")
        if out.dtype != torch.float32 or out.numel() != n * 3 * _lib.IMG * _lib.IMG:
            raise _lib.SvxError("out has the wrong dtype/size")
    m = (ctypes.c_float * 3)(*mean)
    rc = lib.svx_rasterize(records.data_ptr(), n, out.data_ptr(), lay, m, _stream_ptr(records.device))
    _lib.check(rc, "svx_rasterize")
    return out


SCAN_FAILED = 0xFFFFFFFF            # SVX_SCAN_FAILED (include/svx.h): d_gap_off[n_aln] when the offsets pass timed out


def check_scan_total(total):
    if total == SCAN_FAILED:
        raise _lib.SvxError("svx_cigar_scan: SVX_SCAN_FAILED (the offsets pass gave up waiting for a tile in front of it, or the CIGAR array holds more words than the caller said)")
    return total


class CigarScanResult:
    """Device-side result of :func:`cigar_scan`."""

    def __init__(self, gaps, gap_off, stats, n_aln, cap):
        self.gaps, self.gap_off, self.stats, self.n_aln, self.cap = gaps, gap_off, stats, n_aln, cap

    def total(self):
        return check_scan_total(int(self.gap_off[self.n_aln].item()) & 0xFFFFFFFF)

    def to_host(self):
        """(gaps structured array sorted by (aln, op), gap_off uint32[n+1], stats int32[n,4])."""
        off = self.gap_off.cpu().numpy().view(np.uint32)
        total = check_scan_total(int(off[self.n_aln]))
        if total > self.cap:
            raise _lib.SvxError(f"cigar_scan: {total} long gaps exceed the capacity {self.cap}")
        raw = self.gaps[: total * 6].cpu().numpy()
        gaps = raw.view(GAP_DTYPE) if total else np.empty(0, GAP_DTYPE)
        return gaps, off, self.stats.cpu().numpy()


FLAT_SCAN_FROM = None               # mean CIGAR words per alignment from which svx_cigar_scan_flat is picked: None = never -- measured (round 5,
                                    # profiles/r05_bench_cigar.json): 600-800 us on the ONT-shaped launch against 520 us of the three-kernel form (a dozen dependent round trips per tile)


def cigar_scan(cigar, cig_off, ref_start, min_sv, gaps_cap=None, mode=None, n_words=None, span_words=None):
    """cigar: int32/uint32 device tensor of packed BAM CIGAR words; cig_off: int64 [n+1];
    ref_start: int32 [n].  See include/svx.h svx_cigar_scan.  ``mode``: "groups" (svx_cigar_scan: four or eight lanes per alignment
    by the launch's mean words per alignment -- "groups4" / "groups8" / "groups4s" / "groups8s" fix the shape (lanes, s: frames shared by the workgroup) --, three launches), "flat" (svx_cigar_scan_flat: one pass over chunks of the flat word array -- ONT /
    assembly-sized alignments), None: by the mean number of words per alignment (SVX_SCAN_MODE overrides).  ``n_words``: an upper
    bound of the offsets' last entry (default: the size of ``cigar``); ``span_words``: the words between the offsets' first and last
    entry where that is less (a window of a larger array), for the choice of the shape."""
    lib = _lib.load()
    for t, nm in ((cigar, "cigar"), (cig_off, "cig_off"), (ref_start, "ref_start")):
        _require_cuda(t, nm)
    if cigar.dtype not in (torch.int32, torch.uint32) or cig_off.dtype != torch.int64 or ref_start.dtype != torch.int32:
        raise _lib.SvxError("cigar must be (u)int32, cig_off int64, ref_start int32")
    n = ref_start.numel()
    if cig_off.numel() != n + 1:
        raise _lib.SvxError("cig_off must have n_aln + 1 entries")
    dev = cigar.device
    auto = gaps_cap is None
    if auto:
        gaps_cap = max(1024, n // 2)
    gaps = torch.empty(gaps_cap * 6, dtype=torch.int32, device=dev)
    gap_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
    stats = torch.empty((n, 4), dtype=torch.int32, device=dev)
    words = int(cigar.numel()) if n_words is None else int(n_words)
    if mode is None:
        import os
        mode = os.environ.get("SVX_SCAN_MODE") or ("flat" if n and FLAT_SCAN_FROM is not None and words >= FLAT_SCAN_FROM * n else "groups")
    if mode == "flat":
        ws_bytes = int(lib.svx_cigar_scan_flat_ws_bytes(words))
        ws = torch.empty(max(8, ws_bytes), dtype=torch.uint8, device=dev)
        rc = lib.svx_cigar_scan_flat(cigar.data_ptr(), cig_off.data_ptr(), ref_start.data_ptr(), n, words, int(min_sv),
                                     gaps.data_ptr(), gaps_cap, gap_off.data_ptr(), stats.data_ptr(), ws.data_ptr(), int(ws.numel()),
                                     _stream_ptr(dev))
        _lib.check(rc, "svx_cigar_scan_flat")
    else:
        ws = torch.empty(max(16, lib.svx_cigar_scan_ws_bytes(n, words)), dtype=torch.uint8, device=dev)
        flags = {"groups": 0, "groups4": 1 | 8, "groups8": 2 | 8, "groups4s": 1 | 4, "groups8s": 2 | 4}[mode]      # SVX_SCAN_LANES4/8 | SVX_SCAN_(UN)SHARED: the count pass's shape, never a result
        if mode == "groups" and span_words is not None and n:        # a window of a larger array: the library's own rule (svx_cigar.hip SHORT_MEAN / SHARE_MEAN) on the window's words
            flags = (1 if span_words <= 256 * n else 2) | (4 if span_words > 1024 * n else 8)
        rc = lib.svx_cigar_scan(cigar.data_ptr(), cig_off.data_ptr(), ref_start.data_ptr(), n, words, int(min_sv),
                                gaps.data_ptr(), gaps_cap, gap_off.data_ptr(), stats.data_ptr(), ws.data_ptr(), int(ws.numel()), flags,
                                _stream_ptr(dev))
        _lib.check(rc, "svx_cigar_scan")
    res = CigarScanResult(gaps, gap_off, stats, n, gaps_cap)
    if auto and res.total() > gaps_cap:       # d_gap_off[n] holds the full count: rerun with the exact capacity
        return cigar_scan(cigar, cig_off, ref_start, min_sv, gaps_cap=res.total(), mode=mode, n_words=n_words, span_words=span_words)
    return res


def _check_live(live):
    """``live``: None, or a one-element int32 device tensor (:func:`image_dedup`): the leading rows a *_live kernel computes."""
    if live is not None and (not live.is_cuda or live.dtype != torch.int32 or live.numel() != 1):
        raise _lib.SvxError("live must be a one-element int32 device tensor")
    return live.data_ptr() if live is not None else None


def image_dedup(records, keys=False):
    """records int32 [n,12] -> (unique int32 [n,12], inv int32 [n], live int32 [1]) device tensors: the first occurrence of
    every distinct image in input order (rows >= live repeat record 0), the row of ``unique`` that holds each record's
    image, and the number of distinct images -- all on the device, no synchronisation.  ``keys=True``: also the exact
    128-bit image keys, int32 [n,4].  See include/svx.h svx_image_dedup."""
    lib = _lib.load()
    _require_cuda(records, "records")
    if records.dtype != torch.int32 or records.dim() != 2 or records.shape[1] != 12:
        raise _lib.SvxError("records must be int32 [n,12]")
    n, dev = records.shape[0], records.device
    unique = torch.empty((n, 12), dtype=torch.int32, device=dev)
    inv = torch.empty(n, dtype=torch.int32, device=dev)
    live = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    k = torch.empty((n, 4), dtype=torch.int32, device=dev) if keys else None
    rc = lib.svx_image_dedup(records.data_ptr(), n, unique.data_ptr(), inv.data_ptr(), live.data_ptr(),
                             k.data_ptr() if keys else None, ws.data_ptr(), _stream_ptr(dev))
    _lib.check(rc, "svx_image_dedup")
    return (unique, inv, live, k) if keys else (unique, inv, live)


def gather_rows(src, inv, out=None):
    """out[i] = src[inv[i]]: float32 [m,w] rows, inv int32 [n] -> float32 [n,w].  See include/svx.h svx_gather_rows."""
    lib = _lib.load()
    _require_cuda(src, "src")
    _require_cuda(inv, "inv")
    if src.dtype != torch.float32 or src.dim() != 2 or inv.dtype != torch.int32 or inv.dim() != 1:
        raise _lib.SvxError("src must be float32 [m,w] and inv int32 [n]")
    n, w = inv.shape[0], src.shape[1]
    if out is None:
        out = torch.empty((n, w), dtype=torch.float32, device=src.device)
    elif tuple(out.shape) != (n, w) or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.SvxError("out must be a contiguous float32 [n,w] tensor")
    rc = lib.svx_gather_rows(src.data_ptr(), inv.data_ptr(), out.data_ptr(), n, w, _stream_ptr(src.device))
    _lib.check(rc, "svx_gather_rows")
    return out


def bias_relu_pool_lrn(x, bias, lrn=True, radius=2, alpha=2e-05, beta=0.75, k=1.0, active_rows=None, background=None, live=None):
    """x: float32 C8 [n,C/8,H,W,8] raw conv output -> relu(x+bias) -> max-pool 3x3/2 -> (LRN) as one kernel, C8 out.
    ``active_rows`` (int32 [n,H] row masks) + ``background`` (C8 [C/8,H,W,8]): pixels whose bit is clear are read from the
    background instead of ``x`` (an active-set convolution that did not write them).  ``live``: rows >= live are skipped
    (:func:`image_dedup`).  See include/svx.h svx_bias_relu_pool_lrn."""
    lib = _lib.load()
    _require_cuda(x, "x")
    _require_cuda(bias, "bias")
    if x.dtype != torch.float32 or x.dim() != 5 or x.shape[4] != 8 or bias.dtype != torch.float32 or bias.numel() != x.shape[1] * 8:
        raise _lib.SvxError("x must be float32 C8 [n,C/8,H,W,8] and bias float32 [C]")
    n, o, h, w, _e = x.shape
    y = torch.empty((n, o, (h - 3) // 2 + 1, (w - 3) // 2 + 1, 8), dtype=torch.float32, device=x.device)
    if (active_rows is None) != (background is None):
        raise _lib.SvxError("active_rows and background go together")
    if active_rows is not None:
        _require_cuda(active_rows, "active_rows")
        _require_cuda(background, "background")
        if active_rows.dtype != torch.int32 or tuple(active_rows.shape) != (n, h) or background.dtype != torch.float32 \
                or tuple(background.shape)[-4:] != (o, h, w, 8) or background.numel() != o * h * w * 8 \
                or not background.is_contiguous() or not active_rows.is_contiguous():
            raise _lib.SvxError("active_rows must be int32 [n,H] and background float32 C8 [C/8,H,W,8]")
    rc = lib.svx_bias_relu_pool_lrn_live(x.data_ptr(), bias.data_ptr(), y.data_ptr(), n, o * 8, h, w, 1 if lrn else 0, radius,
                                         alpha, beta, k, active_rows.data_ptr() if active_rows is not None else None,
                                         background.data_ptr() if background is not None else None, _check_live(live),
                                         _stream_ptr(x.device))
    _lib.check(rc, "svx_bias_relu_pool_lrn")
    return y


def encode_conv1(records, w1_hwio, base, lrn=True, radius=2, alpha=2e-05, beta=0.75, k=1.0, touched=False, live=None):
    """records int32 [n,12] -> float32 C8 [n,12,27,27,8]: rasterise + conv1 + relu + pool1 + norm1 in one
    kernel, exploiting the sparsity of the similarity image.  See include/svx.h svx_encode_conv1.
    ``touched=True``: also return the int32 [n,27] row masks of the pooled pixels with a set tap under them.
    ``live``: rows >= live are skipped (:func:`image_dedup`)."""
    lib = _lib.load()
    for t, nm in ((records, "records"), (w1_hwio, "w1"), (base, "base")):
        _require_cuda(t, nm)
    if records.dtype != torch.int32 or records.dim() != 2 or records.shape[1] != 12:
        raise _lib.SvxError("records must be int32 [n,12]")
    if tuple(w1_hwio.shape) != (11, 11, 3, 96) or w1_hwio.dtype != torch.float32 or base.numel() != 96:
        raise _lib.SvxError("w1 must be float32 HWIO [11,11,3,96] and base float32 [96]")
    n = records.shape[0]
    y = torch.empty((n, 12, 27, 27, 8), dtype=torch.float32, device=records.device)
    mask = torch.empty((n, 27), dtype=torch.int32, device=records.device) if touched else None
    rc = lib.svx_encode_conv1_live(records.data_ptr(), n, w1_hwio.data_ptr(), base.data_ptr(), y.data_ptr(), 1 if lrn else 0,
                                   radius, alpha, beta, k, mask.data_ptr() if touched else None, _check_live(live),
                                   _stream_ptr(records.device))
    _lib.check(rc, "svx_encode_conv1")
    return (y, mask) if touched else y


def alexnet_active_sets(touched, totals=None, rows=False, live=None):
    """touched int32 [n,27] (encode_conv1) -> (list2 [n*729], list3, list4, list5 [n*169], counts [4]) int32 device
    tensors: the output pixels of conv2..conv5 that can differ from the response to an empty image.
    ``totals``: optional int64 device tensor [5] the launch adds its executed pixel counts (conv2..conv5) and image count to.
    ``live``: the lists cover the leading ``live`` images only (:func:`image_dedup`).
    See include/svx.h svx_alexnet_active_sets."""
    lib = _lib.load()
    _require_cuda(touched, "touched")
    if totals is not None and (not totals.is_cuda or totals.dtype != torch.int64 or totals.numel() != 5):
        raise _lib.SvxError("totals must be an int64 device tensor [5]")
    if touched.dtype != torch.int32 or touched.dim() != 2 or touched.shape[1] != 27:
        raise _lib.SvxError("touched must be int32 [n,27]")
    n, dev = touched.shape[0], touched.device
    lists = [torch.empty(n * hw, dtype=torch.int32, device=dev) for hw in (729, 169, 169, 169)]
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    ws = torch.empty(max(n, 1) * 4, dtype=torch.int32, device=dev)
    active2 = torch.empty((n, 27), dtype=torch.int32, device=dev) if rows else None
    rc = lib.svx_alexnet_active_sets_live(touched.data_ptr(), n, lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(),
                                          lists[3].data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                          totals.data_ptr() if totals is not None else None,
                                          active2.data_ptr() if rows else None, _check_live(live), _stream_ptr(dev))
    _lib.check(rc, "svx_alexnet_active_sets")
    if rows:                                                  # + int32 [n,27] row masks of conv2's active pixels
        return lists[0], lists[1], lists[2], lists[3], counts, active2
    return lists[0], lists[1], lists[2], lists[3], counts


def conv2d_same(x, w_packed, bias=None, groups=1, relu=False, pixels=None, pixel_count=None, out=None, background=None, live=None):
    """x float32 C8 [n,Cin/8,H,W,8], w_packed float32 [k,k,Cin/groups/8,Cout,8] (:func:`pack_conv_weights`) -> C8
    [n,Cout/8,H,W,8]: stride-1 SAME convolution on the fp32 matrix cores, optional fused bias + ReLU.
    ``pixels`` / ``pixel_count`` (device int32 permutation of the pixel ids and the number of leading active entries,
    a one-element view): compute only the active output pixels; the others receive ``background`` (C8 [Cout/8,H,W,8]) or,
    without it, keep what ``out`` holds.  ``live`` (list mode): the lists cover the leading ``live`` images only
    (:func:`alexnet_active_sets`).  See include/svx.h svx_conv2d_same."""
    lib = _lib.load()
    _require_cuda(x, "x")
    _require_cuda(w_packed, "w_packed")
    if x.dtype != torch.float32 or x.dim() != 5 or x.shape[4] != 8 or w_packed.dtype != torch.float32 or w_packed.dim() != 5 or w_packed.shape[4] != 8:
        raise _lib.SvxError("x must be float32 C8 [n,C/8,H,W,8] and w float32 packed [k,k,cin_g/8,cout,8]")
    n, cin8, h, w, _e = x.shape
    cin = cin8 * 8
    k, k2, cin_g8, cout, _e2 = w_packed.shape
    if k != k2 or cin_g8 * 8 * groups != cin:
        raise _lib.SvxError("weight shape %s does not match input %s with %d groups" % (tuple(w_packed.shape), tuple(x.shape), groups))
    if bias is not None:
        _require_cuda(bias, "bias")
    if (pixels is None) != (pixel_count is None) or (pixels is not None and out is None and background is None):
        raise _lib.SvxError("pixels and pixel_count go together, with out or background")
    if live is not None and pixels is None:
        raise _lib.SvxError("live needs pixels")
    if background is not None and (pixels is None or tuple(background.shape[-4:]) != (cout // 8, h, w, 8) or not background.is_contiguous()):
        raise _lib.SvxError("background must be a contiguous float32 C8 [Cout/8,H,W,8] tensor and needs pixels")
    y = out if out is not None else torch.empty((n, cout // 8, h, w, 8), dtype=torch.float32, device=x.device)
    if tuple(y.shape) != (n, cout // 8, h, w, 8) or y.dtype != torch.float32 or not y.is_contiguous():
        raise _lib.SvxError("out must be a contiguous float32 C8 [n,Cout/8,H,W,8] tensor")
    rc = lib.svx_conv2d_same_live(x.data_ptr(), w_packed.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(),
                                  n, cin, cout, h, w, k, groups, 1 if relu else 0,
                                  pixels.data_ptr() if pixels is not None else None,
                                  pixel_count.data_ptr() if pixel_count is not None else None,
                                  background.data_ptr() if background is not None else None, _check_live(live),
                                  _stream_ptr(x.device))
    _lib.check(rc, "svx_conv2d_same")
    return y


def pack_fc_weights(w_out_in):
    """fc weights [out,in] -> [out/32, in/8, 32, 8] (svx_fc_bias_act's d_w_packed)."""
    n, k = w_out_in.shape
    if n % 32 or k % 8:
        raise _lib.SvxError("fc weights need out % 32 == 0 and in % 8 == 0")
    return w_out_in.reshape(n // 32, 32, k // 8, 8).permute(0, 2, 1, 3).contiguous()


def fc_bias_act(x, w_packed, bias, relu=True, out=None, ws=None, live=None):
    """x float32 [m,k], w_packed [n/32,k/8,32,8] (:func:`pack_fc_weights`), bias [n] -> act(x @ W^T + bias) [m,n] on the
    fp32 matrix cores (split-K wave tiles + ordered reduction).  ``live``: rows >= live are skipped; the split-K grouping
    stays that of m.  See include/svx.h svx_fc_bias_act."""
    lib = _lib.load()
    for t, nm in ((x, "x"), (w_packed, "w_packed"), (bias, "bias")):
        _require_cuda(t, nm)
    if x.dtype != torch.float32 or x.dim() != 2 or w_packed.dim() != 4 or w_packed.shape[2:] != (32, 8) or w_packed.shape[1] * 8 != x.shape[1]:
        raise _lib.SvxError("x must be float32 [m,k] and w packed [n/32,k/8,32,8]")
    m, k = x.shape
    n = w_packed.shape[0] * 32
    if bias.numel() != n:
        raise _lib.SvxError("bias must have n entries")
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    need = lib.svx_fc_ws_bytes(m, n, k)
    if ws is None or ws.numel() * ws.element_size() < need:
        ws = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=x.device)
    rc = lib.svx_fc_bias_act_live(x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr(), ws.data_ptr(), m, n, k,
                                  1 if relu else 0, _check_live(live), _stream_ptr(x.device))
    _lib.check(rc, "svx_fc_bias_act")
    return out


def fc8_softmax(x, w_out_in, bias, out=None, live=None):
    """x float32 [n,4096], w float32 [5,4096], bias [5] -> packed float32 [n,12] = softmax[5], class, logits[5], 0.
    ``live``: rows >= live are skipped.  See include/svx.h svx_fc8_softmax."""
    lib = _lib.load()
    for t, nm in ((x, "x"), (w_out_in, "w"), (bias, "bias")):
        _require_cuda(t, nm)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != 4096 or tuple(w_out_in.shape) != (5, 4096):
        raise _lib.SvxError("x must be float32 [n,4096] and w float32 [5,4096]")
    n = x.shape[0]
    if out is None:
        out = torch.empty((n, 12), dtype=torch.float32, device=x.device)
    rc = lib.svx_fc8_softmax_live(x.data_ptr(), w_out_in.data_ptr(), bias.data_ptr(), out.data_ptr(), n, _check_live(live),
                                  _stream_ptr(x.device))
    _lib.check(rc, "svx_fc8_softmax")
    return out


def fc_partial(x, w_packed, live=None):
    """The split-K half of :func:`fc_bias_act`: x float32 [m,k], w_packed [n/32,k/8,32,8] -> the partial sums float32
    [splits,m,n] (rows >= live are skipped), to be added up in order by :func:`fc8_tail`.  See include/svx.h svx_fc_partial_live."""
    lib = _lib.load()
    for t, nm in ((x, "x"), (w_packed, "w_packed")):
        _require_cuda(t, nm)
    if x.dtype != torch.float32 or x.dim() != 2 or w_packed.dim() != 4 or w_packed.shape[2:] != (32, 8) or w_packed.shape[1] * 8 != x.shape[1]:
        raise _lib.SvxError("x must be float32 [m,k] and w packed [n/32,k/8,32,8]")
    m, k = x.shape
    n = w_packed.shape[0] * 32
    part = torch.empty((lib.svx_fc_splits(m, n, k), m, n), dtype=torch.float32, device=x.device)
    rc = lib.svx_fc_partial_live(x.data_ptr(), w_packed.data_ptr(), part.data_ptr(), m, n, k, _check_live(live), _stream_ptr(x.device))
    _lib.check(rc, "svx_fc_partial")
    return part


def fc8_tail(part, bias7, w_out_in, bias, inv, out=None, live=None):
    """part float32 [splits,m,4096] (fc7's partial sums, :func:`fc_partial`), bias7 [4096], w [5,4096], bias [5], inv int32 [n]
    -> packed float32 [n,12]: relu(bias7 + the splits in order), fc8 + softmax per live row, and each row written to the
    records whose image it is -- fc7's reduction, :func:`fc8_softmax` and :func:`gather_rows` in one launch.  See include/svx.h
    svx_fc8_tail_live."""
    lib = _lib.load()
    for t, nm in ((part, "part"), (bias7, "bias7"), (w_out_in, "w"), (bias, "bias"), (inv, "inv")):
        _require_cuda(t, nm)
    if part.dtype != torch.float32 or part.dim() != 3 or part.shape[2] != 4096 or not part.is_contiguous() or bias7.numel() != 4096 \
            or tuple(w_out_in.shape) != (5, 4096) or inv.dtype != torch.int32 or inv.dim() != 1:
        raise _lib.SvxError("part must be a contiguous float32 [splits,m,4096], bias7 [4096], w float32 [5,4096] and inv int32 [n]")
    splits, m, n = part.shape[0], part.shape[1], inv.shape[0]
    if out is None:
        out = torch.empty((n, 12), dtype=torch.float32, device=part.device)
    elif tuple(out.shape) != (n, 12) or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.SvxError("out must be a contiguous float32 [n,12] tensor")
    rc = lib.svx_fc8_tail_live(part.data_ptr(), splits, bias7.data_ptr(), w_out_in.data_ptr(), bias.data_ptr(), inv.data_ptr(),
                               out.data_ptr(), m, n, _check_live(live), _stream_ptr(part.device))
    _lib.check(rc, "svx_fc8_tail")
    return out


def span_position_distance(starts, ends, part_off, normalizer=1000.0):
    """Condensed span_position_distance matrices of several partitions in one launch.
    starts / ends: float64 device tensors [N] (partitions concatenated); part_off: int sequence [P+1].
    -> (float64 device tensor [sum n_p (n_p - 1) / 2] in scipy pdist order, out_off numpy uint64 [P+1]).
    See include/svx.h svx_span_position_distance."""
    lib = _lib.load()
    _require_cuda(starts, "starts")
    _require_cuda(ends, "ends")
    if starts.dtype != torch.float64 or ends.dtype != torch.float64 or starts.numel() != ends.numel():
        raise _lib.SvxError("starts / ends must be float64 tensors of one length")
    part = np.ascontiguousarray(part_off, np.uint64)
    if part.ndim != 1 or part.size < 1 or int(part[-1]) != starts.numel() or np.any(np.diff(part.astype(np.int64)) < 0):
        raise _lib.SvxError("part_off must be ascending and end at the number of signatures")
    sizes = np.diff(part.astype(np.int64))
    out_off = np.zeros(part.size, np.uint64)
    out_off[1:] = np.cumsum(sizes * (sizes - 1) // 2)
    total = int(out_off[-1])
    out = torch.empty(total, dtype=torch.float64, device=starts.device)
    if total:
        d_part = torch.from_numpy(part.view(np.int64)).to(starts.device)
        d_off = torch.from_numpy(out_off.view(np.int64)).to(starts.device)
        rc = lib.svx_span_position_distance(starts.data_ptr(), ends.data_ptr(), d_part.data_ptr(), part.size - 1, d_off.data_ptr(), total,
                                            float(normalizer), out.data_ptr(), _stream_ptr(starts.device))
        _lib.check(rc, "svx_span_position_distance")
    return out, out_off


HASH_MAX_X = 2048                    # longest piece of svx_hash_seeds
HASH_LONG_MAX_X = 65536              # longest piece of svx_hash_seeds_long (x's k-mers in tiles, --max_hash_len raised)
_BASE_CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGTNacgtnRYKMS"):
    _BASE_CODE[_c] = _i
HASH_JOB_DTYPE = np.dtype([("x_off", "<u8"), ("y_off", "<u8"), ("x_len", "<u4"), ("y_len", "<u4"), ("table_off", "<u8"),
                           ("table_slots", "<u4"), ("hit_cap", "<u4"), ("hit_off", "<u8")])


def pack_bases(seq):
    """str / bytes over ACGTN, acgtn (soft-masked references) and RYKMS -> uint8 symbols 0..14, or None when another
    character occurs (those jobs take the host path, whose k-mers are the raw strings)."""
    raw = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), np.uint8)
    codes = _BASE_CODE[raw]
    return None if (codes == 255).any() else codes


HASH_BUDGET = 4 << 30                # bytes of scratch table + hit lists one launch may ask for (a 20 kb window: 6.5 MB; 233 jobs on
                                     # windows of 10-19 kb, the jobs of a 1 Mb HiFi window: ~1.3 GB -- one launch)
HASH_PACKED_ROWS = 4096              # rows the first pack of a launch has room for (a window's jobs return a few hundred)


def hash_job_arrays(jobs):
    """[(x_codes, y_codes), ...] -> (bases uint8: all sequences end to end, desc int64 [n,4] = x_off, x_len, y_off, y_len):
    the form :func:`hash_seeds_async` takes and the helpers' pipe carries."""
    desc = np.zeros((len(jobs), 4), np.int64)
    lens = np.fromiter((len(s) for job in jobs for s in job), np.int64, 2 * len(jobs))
    offs = np.cumsum(lens) - lens
    desc[:, 0], desc[:, 1], desc[:, 2], desc[:, 3] = offs[0::2], lens[0::2], offs[1::2], lens[1::2]
    parts = [s for job in jobs for s in job]
    return (np.concatenate(parts).astype(np.uint8, copy=False) if parts else np.zeros(0, np.uint8)), desc


def hash_hit_caps(desc):
    """Capacity of each of a job's two hit lists (a count above it: the job is redone on the host)."""
    return 4 * np.asarray(desc, np.int64).reshape(-1, 4)[:, 3] + 64


def hash_split_rows(desc, counts, row_off, rows):
    """What a finished :class:`HashSeedsHandle` returns -> list of (hits_a, hits_b) int32 [n,4] per job, None for a job
    with an overflowed list."""
    counts = np.asarray(counts, np.int64)
    cap = hash_hit_caps(desc)
    if counts.size != 2 * cap.size or len(row_off) != counts.size + 1:
        raise _lib.SvxError("hash_split_rows: %d counts / %d offsets for %d jobs" % (counts.size, len(row_off), cap.size))
    rows = np.asarray(rows, np.int32).reshape(-1, 4)
    off = np.asarray(row_off, np.int64).tolist()
    if off[-1] != len(rows):
        raise _lib.SvxError("hash_split_rows: %d rows where the offsets end at %d" % (len(rows), off[-1]))
    over = ((counts[0::2] > cap) | (counts[1::2] > cap)).tolist()
    return [None if over[j] else (rows[off[2 * j]:off[2 * j + 1]], rows[off[2 * j + 1]:off[2 * j + 2]]) for j in range(cap.size)]


_HASH_STREAMS = {}


def _hash_stream(dev):
    """The re-aligner's own stream on ``dev``: its uploads, launches and read-backs wait for no other stream's work."""
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _HASH_STREAMS:
        _HASH_STREAMS[key] = torch.cuda.Stream(dev)
    return _HASH_STREAMS[key]


class _HashLaunch:
    """One launch of a :class:`HashSeedsHandle` under way: jobs [lo, lo + m) of the batch, its output array on the device
    (counts [2 m], row_off [2 m + 1], padding to ``hdr`` words, then ``rows`` packed rows), and the read-back of it."""
    __slots__ = ("index", "lo", "m", "hdr", "rows", "d_out", "h_out", "event")

    def __init__(self, index, lo, m, hdr, rows, d_out):
        self.index, self.lo, self.m, self.hdr, self.rows, self.d_out = index, lo, m, hdr, rows, d_out
        self.h_out = self.event = None


class HashSeedsHandle:
    """A batch of re-aligner jobs under way on the device (:func:`hash_seeds_async`).  ``done()`` never blocks;
    ``result()`` waits -> (counts uint32 [2 n], row_off uint32 [2 n + 1], rows int32 [total, 4]): the lists A0 B0 A1 B1 ...
    compacted (``svx_hash_pack_hits``), to be cut up by :func:`hash_split_rows`.  ``launches``: seed launches so far.

    A batch whose scratch table and hit lists exceed ``budget`` bytes runs as several launches over one scratch area; the
    next is enqueued when the host has seen that the rows of the one before fitted its packed array (otherwise the pack,
    not the seeds, is repeated with a larger one).  A single launch -- a window's jobs -- is enqueued whole: upload,
    seeds, pack, download, one event.

    ``max_piece`` above :data:`HASH_MAX_X` (up to :data:`HASH_LONG_MAX_X`) admits longer pieces: they run through
    ``svx_hash_seeds_long`` in the same launches' index space, with a workspace from the same stream's pool that counts
    under ``budget``."""

    def __init__(self, bases, desc, k, window, device, budget=HASH_BUDGET, packed_rows=HASH_PACKED_ROWS, max_piece=HASH_MAX_X):
        self._lib = _lib.load()
        dev = self._dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.SvxError("hash_seeds: needs a device (got %s); the hot path has no CPU fallback" % (dev,))
        bases = np.ascontiguousarray(bases, np.uint8).reshape(-1)
        desc = np.ascontiguousarray(desc, np.int64).reshape(-1, 4)
        n = self._n = len(desc)
        self._k, self._window, self._packed_rows = int(k), int(window), max(1, int(packed_rows))
        self.launches = 0
        self._parts, self._cur, self._result = [], None, None
        x_off, x_len, y_off, y_len = (desc[:, c] for c in range(4))
        if n and ((desc < 0).any() or (x_off + x_len > bases.size).any() or (y_off + y_len > bases.size).any()):
            raise _lib.SvxError("hash_seeds: a job's sequence lies outside the base array")
        max_piece = self._max_piece = int(max_piece)
        if not HASH_MAX_X <= max_piece <= HASH_LONG_MAX_X:
            raise _lib.SvxError("hash_seeds: max_piece %d outside %d..%d" % (max_piece, HASH_MAX_X, HASH_LONG_MAX_X))
        if n and int(x_len.max()) > max_piece:
            raise _lib.SvxError("hash_seeds: piece longer than %d bases" % max_piece)
        if n and int(y_len.max()) >= 1 << 26:
            raise _lib.SvxError("hash_seeds: window longer than 2^26 bases")
        if n == 0:
            self._result = (np.zeros(0, np.uint32), np.zeros(1, np.uint32), np.zeros((0, 4), np.int32))
            return
        want = 8 * np.maximum(y_len, 1)
        slots = np.left_shift(1, np.ceil(np.log2(want)).astype(np.int64))          # power of two >= 8 * len(y)
        slots = np.where(slots < want, slots * 2, slots)
        cap = hash_hit_caps(desc)
        is_long = x_len > HASH_MAX_X                                       # svx_hash_seeds_long's jobs and their workspace
        ws = np.where(is_long, (16 * x_len + 4 * y_len + 15) // 16 * 16, 0)
        cost = (slots + 2 * cap) * 16 + ws
        # consecutive jobs to a launch while they fit the budget (a job larger than it goes alone)
        self._chunks, lo, used = [], 0, 0
        for j, c in enumerate(cost.tolist()):
            if j > lo and used + c > budget:
                self._chunks.append((lo, j))
                lo, used = j, 0
            used += c
        self._chunks.append((lo, n))
        jd = np.zeros(n, HASH_JOB_DTYPE)
        jd["x_off"], jd["x_len"], jd["y_off"], jd["y_len"], jd["table_slots"], jd["hit_cap"] = x_off, x_len, y_off, y_len, slots, cap
        ws_off = np.zeros(n, np.uint64)
        max_slots = max_rows = max_ws = 0
        for lo, hi in self._chunks:
            jd["table_off"][lo:hi] = np.cumsum(slots[lo:hi]) - slots[lo:hi]
            jd["hit_off"][lo:hi] = 2 * (np.cumsum(cap[lo:hi]) - cap[lo:hi])
            ws_off[lo:hi] = np.cumsum(ws[lo:hi]) - ws[lo:hi]
            max_slots, max_rows = max(max_slots, int(slots[lo:hi].sum())), max(max_rows, 2 * int(cap[lo:hi].sum()))
            max_ws = max(max_ws, int(ws[lo:hi].sum()))
        self._long = [bool(is_long[lo:hi].any()) for lo, hi in self._chunks]
        self._stream = _hash_stream(dev)
        raw = jd.view(np.uint8).reshape(-1)
        if max_ws:                                                      # the workspace offsets ride behind the job records
            raw = np.concatenate([raw, ws_off.view(np.uint8)])
        self._ws_at = HASH_JOB_DTYPE.itemsize * n                      # (read only by a launch with a long job: then they were appended)
        with torch.cuda.stream(self._stream):
            # one pinned staging buffer, one upload: the job records (SvxHashJob), then the bases (+ 16 bytes of slack)
            self._h_in = torch.empty(raw.size + bases.size + 16, dtype=torch.uint8, pin_memory=True)
            h = self._h_in.numpy()
            h[:raw.size], h[raw.size:raw.size + bases.size], h[raw.size + bases.size:] = raw, bases, 0
            self._d_in = torch.empty(self._h_in.numel(), dtype=torch.uint8, device=dev)
            self._d_in.copy_(self._h_in, non_blocking=True)
            self._d_table = torch.empty(2 * max_slots, dtype=torch.int64, device=dev)
            self._d_hits = torch.empty(4 * max_rows, dtype=torch.int32, device=dev)
            self._d_ws = torch.empty(max_ws, dtype=torch.uint8, device=dev) if max_ws else None
        self._bases_at = raw.size
        self._start(0)

    def _start(self, ci):
        lo, hi = self._chunks[ci]
        m = hi - lo
        hdr = (4 * m + 1 + 3) // 4 * 4                                 # counts [2 m], row_off [2 m + 1], then 16-byte aligned rows
        with torch.cuda.stream(self._stream):
            d_out = torch.empty(hdr + 4 * self._packed_rows, dtype=torch.int32, device=self._dev)
            sp = ctypes.c_void_p(self._stream.cuda_stream)
            rc = self._lib.svx_hash_seeds(self._d_in.data_ptr() + self._bases_at, self._d_in.data_ptr() + HASH_JOB_DTYPE.itemsize * lo, m, self._d_table.data_ptr(),
                                          self._d_hits.data_ptr(), d_out.data_ptr(), self._k, self._window, HASH_MAX_X, sp)
            _lib.check(rc, "svx_hash_seeds")
            if self._long[ci]:                                          # the same jobs: each kernel leaves the other's alone
                rc = self._lib.svx_hash_seeds_long(self._d_in.data_ptr() + self._bases_at, self._d_in.data_ptr() + HASH_JOB_DTYPE.itemsize * lo, m,
                                                   self._d_table.data_ptr(), self._d_hits.data_ptr(), d_out.data_ptr(), self._d_ws.data_ptr(),
                                                   self._d_in.data_ptr() + self._ws_at + 8 * lo, self._k, self._window, self._max_piece, sp)
                _lib.check(rc, "svx_hash_seeds_long")
            self.launches += 1
        self._cur = _HashLaunch(ci, lo, m, hdr, self._packed_rows, d_out)
        self._pack()

    def _pack(self):
        """Pack the current launch's lists into its output array and read that back (again, after the array has grown)."""
        cur = self._cur
        with torch.cuda.stream(self._stream):
            sp = ctypes.c_void_p(self._stream.cuda_stream)
            out = cur.d_out.data_ptr()
            rc = self._lib.svx_hash_pack_hits(self._d_in.data_ptr() + HASH_JOB_DTYPE.itemsize * cur.lo, cur.m, self._d_hits.data_ptr(), out,
                                              out + 4 * 2 * cur.m, out + 4 * cur.hdr, cur.rows, sp)
            _lib.check(rc, "svx_hash_pack_hits")
            cur.h_out = torch.empty(cur.d_out.numel(), dtype=torch.int32, pin_memory=True)
            cur.h_out.copy_(cur.d_out, non_blocking=True)
            cur.event = torch.cuda.Event()
            cur.event.record(self._stream)

    def _advance(self):
        """The launch under way has finished: keep its rows (or pack again into a larger array), start the next."""
        cur = self._cur
        m, hdr = cur.m, cur.hdr
        h = cur.h_out.numpy()
        total = int(h[4 * m]) & 0xFFFFFFFF
        if total > cur.rows:
            with torch.cuda.stream(self._stream):
                bigger = torch.empty(hdr + 4 * total, dtype=torch.int32, device=self._dev)
                bigger[:2 * m].copy_(cur.d_out[:2 * m])                 # the counts: the pack reads them from its output array
            cur.rows, cur.d_out = total, bigger
            self._pack()
            return
        self._parts.append((h[:2 * m].view(np.uint32).copy(), h[2 * m:4 * m + 1].view(np.uint32).copy(), h[hdr:hdr + 4 * total].reshape(-1, 4).copy()))
        self._cur = None
        if cur.index + 1 < len(self._chunks):
            self._start(cur.index + 1)
            return
        counts = np.concatenate([p[0] for p in self._parts])
        row_off = np.zeros(2 * self._n + 1, np.uint32)
        at = base = 0
        for _c, off, _r in self._parts:
            row_off[at:at + off.size] = off + np.uint32(base)
            at, base = at + off.size - 1, base + int(off[-1])
        self._result = (counts, row_off, np.concatenate([p[2] for p in self._parts]))
        self._parts = self._d_in = self._h_in = self._d_table = self._d_hits = self._d_ws = None

    def done(self):
        while self._result is None and self._cur.event.query():
            self._advance()
        return self._result is not None

    def result(self):
        while self._result is None:
            self._cur.event.synchronize()
            self._advance()
        return self._result


def hash_seeds_async(bases_u8, job_desc, k, window, device, budget=HASH_BUDGET, packed_rows=HASH_PACKED_ROWS, max_piece=HASH_MAX_X):
    """One contiguous array of packed bases (pack_bases symbols) + int64 [n,4] job descriptors (x_off, x_len, y_off, y_len:
    :func:`hash_job_arrays`) -> :class:`HashSeedsHandle`.  Upload, ``svx_hash_seeds``, ``svx_hash_pack_hits`` and the
    read-back of the packed rows are enqueued on the re-aligner's own stream, through pinned memory (a pageable copy
    would wait behind the CNN's queued launches, see Sample.from_table); nothing here waits for another stream.
    ``max_piece``: the longest piece admitted (default: the short kernel's 2048; up to HASH_LONG_MAX_X)."""
    return HashSeedsHandle(bases_u8, job_desc, k, window, device, budget, packed_rows, max_piece)


def hash_seeds(jobs, k, window, device, budget=HASH_BUDGET, packed_rows=HASH_PACKED_ROWS, max_piece=HASH_MAX_X):
    """jobs: list of (x_codes, y_codes) uint8 arrays (pack_bases) -> list of (hits_a, hits_b) int32 arrays [n,4]
    = {y position, x position or position in x's reverse complement, match length, forward}, or None for a job whose
    hit lists overflowed.  The synchronous form of :func:`hash_seeds_async`: one launch for the whole batch unless its
    scratch exceeds ``budget`` bytes (then several, with the same results).  Pieces above 2048 bases are refused unless
    ``max_piece`` admits them (svx_hash_seeds_long).  See include/svx.h svx_hash_seeds."""
    if not jobs:
        return []
    bases, desc = hash_job_arrays(jobs)
    return hash_split_rows(desc, *hash_seeds_async(bases, desc, k, window, device, budget, packed_rows, max_piece).result())


def bgzf_block_table(raw):
    """BGZF bytes (host, uint8 array: a run of whole blocks) -> (src_off uint64 [n], src_len uint32 [n], isize uint32 [n],
    block_off uint64 [n]): where every block's DEFLATE payload lies, its inflated size, and the block's own offset."""
    raw = np.ascontiguousarray(raw, np.uint8)
    src_off, src_len, isize, block_off = [], [], [], []
    p, n = 0, raw.size
    while p + 18 <= n:
        if not (raw[p] == 0x1f and raw[p + 1] == 0x8b and raw[p + 2] == 8 and raw[p + 3] & 4):
            raise _lib.SvxError("not a BGZF block at offset %d" % p)
        xlen = int(raw[p + 10]) | int(raw[p + 11]) << 8
        q, bsize = p + 12, None
        while q + 4 <= p + 12 + xlen:
            slen = int(raw[q + 2]) | int(raw[q + 3]) << 8
            if raw[q] == 66 and raw[q + 1] == 67:
                bsize = int(raw[q + 4]) | int(raw[q + 5]) << 8
            q += 4 + slen
        if bsize is None or p + bsize + 1 > n:
            break
        end = p + bsize + 1
        block_off.append(p)
        src_off.append(p + 12 + xlen)
        src_len.append(end - 8 - (p + 12 + xlen))
        isize.append(int.from_bytes(raw[end - 4:end].tobytes(), "little"))
        p = end
    return (np.asarray(src_off, np.uint64), np.asarray(src_len, np.uint32), np.asarray(isize, np.uint32), np.asarray(block_off, np.uint64))


WAVE_KERNEL_BELOW = 20_000          # (lane-per-block era) blocks per launch under which the wave-per-block kernel beat the lane-per-block one


def inflate_variant_for(n_blocks):
    """Which inflate implementation a launch of ``n_blocks`` blocks takes: "fast" -- the two-kernel form (svx_inflate2.hip:
    parallel Huffman decoding per block + LZ copies; 0.5 + 0.65 ms per 1,000 blocks, proportional to the launch) -- unless
    SVX_INFLATE_VARIANT names another (lds | private | wave | lane | fast; "auto": the round-3 choice between the lane- and
    the wave-per-block kernel by launch size)."""
    import os
    variant = os.environ.get("SVX_INFLATE_VARIANT", "fast")
    if variant == "auto":
        return "wave" if n_blocks < WAVE_KERNEL_BELOW else "lane"
    return variant


def inflate_workspace(lib, variant, inflated_bytes, n_blocks, device):
    """The workspace tensor a launch of ``variant`` needs (None: none), allocated on the caller's current stream."""
    if not variant.startswith("fast"):
        return None
    return torch.empty(int(lib.svx_bgzf_inflate_fast_ws_bytes(int(inflated_bytes), int(n_blocks))), dtype=torch.uint8, device=device)


def launch_inflate(lib, variant, comp_ptr, src_ptr, len_ptr, dst_ptr, n_blocks, out_ptr, status_ptr, inflated_bytes, device, ws=None, tokens_stream=None):
    """Enqueue one inflate launch on the current stream of ``device``.  ``ws``: the "fast" form's workspace
    (:func:`inflate_workspace`); None: taken from the caching allocator here -- stream-ordered, so it may die with this call.
    ``tokens_stream``: the "fast" form's first kernel goes there (svx_bgzf_inflate_fast_on), the rest stays on the current stream."""
    st = _stream_ptr(device)
    lz = None
    if variant in ("fast-lane", "fast-wave", "fast-table"):   # the "fast" form with its LZ kernel by name (tests, measurements)
        lz, variant = variant[5:], "fast"
    if variant == "fast":
        d_ws = ws if ws is not None else inflate_workspace(lib, variant, inflated_bytes, n_blocks, device)
        ws_bytes = int(d_ws.numel())
        rc = _launch_fast(lib, comp_ptr, src_ptr, len_ptr, dst_ptr, n_blocks, inflated_bytes, out_ptr, status_ptr, d_ws, ws_bytes, tokens_stream, st, lz)
        _lib.check(rc, "svx_bgzf_inflate (%s)" % variant)
        return
    fn = {"lds": lib.svx_bgzf_inflate_lds, "private": lib.svx_bgzf_inflate_private, "wave": lib.svx_bgzf_inflate_wave,
          "lane": lib.svx_bgzf_inflate}[variant]
    rc = fn(comp_ptr, src_ptr, len_ptr, dst_ptr, n_blocks, out_ptr, status_ptr, st)
    _lib.check(rc, "svx_bgzf_inflate (%s)" % variant)


def _launch_fast(lib, comp_ptr, src_ptr, len_ptr, dst_ptr, n_blocks, inflated_bytes, out_ptr, status_ptr, d_ws, ws_bytes, tokens_stream, st, lz=None):
    if lz is not None:                                        # the LZ kernel by name: an argument of the experimental entry point (svx_experimental.h)
        tok = ctypes.c_void_p(tokens_stream.cuda_stream) if tokens_stream is not None else st
        return lib.svx_bgzf_inflate_fast_lz(comp_ptr, src_ptr, len_ptr, dst_ptr, n_blocks, int(inflated_bytes), out_ptr, status_ptr, d_ws.data_ptr(), ws_bytes,
                                            {"lane": 1, "wave": 2, "table": 3}[lz], tok, st)
    if tokens_stream is not None:
        return lib.svx_bgzf_inflate_fast_on(comp_ptr, src_ptr, len_ptr, dst_ptr, n_blocks, int(inflated_bytes), out_ptr, status_ptr, d_ws.data_ptr(), ws_bytes,
                                            ctypes.c_void_p(tokens_stream.cuda_stream), st)
    return lib.svx_bgzf_inflate_fast(comp_ptr, src_ptr, len_ptr, dst_ptr, n_blocks, int(inflated_bytes), out_ptr, status_ptr, d_ws.data_ptr(), ws_bytes, st)


INFLATE_BAD_CRC = 9                 # SVX_INFLATE_BAD_CRC: the block inflated, but not to the bytes its footer's CRC32 was taken of


def bgzf_crc_wanted():
    """BGZF footers are verified (htslib does, behind pysam's fetch) unless SVX_BGZF_CRC=0."""
    import os
    return os.environ.get("SVX_BGZF_CRC", "1") != "0"


def bgzf_inflate(d_comp, src_off, src_len, isize, wave=None, crc=None):
    """d_comp: uint8 device tensor holding the compressed bytes (16-byte aligned, padded to a multiple of 16); src_off / src_len / isize: host
    arrays of :func:`bgzf_block_table` (or the native reader's).  -> (uint8 device tensor with the inflated stream,
    int32 device tensor [n] status: 0 = ok, 9 = CRC32 mismatch).  ``crc``: verify the blocks' footers (svx_bgzf_crc32; default:
    yes unless SVX_BGZF_CRC=0).  See include/svx.h svx_bgzf_inflate."""
    lib = _lib.load()
    _require_cuda(d_comp, "d_comp")
    if d_comp.dtype != torch.uint8:
        raise _lib.SvxError("d_comp must be a uint8 tensor")
    n = int(len(src_off))
    dev = d_comp.device
    dst = np.zeros(n + 1, np.uint64)
    dst[1:] = np.cumsum(np.asarray(isize, np.uint64))
    total = int(dst[-1])
    d_out = torch.empty(max(total, 4), dtype=torch.uint8, device=dev)
    d_status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    if n:
        d_src = torch.from_numpy(np.ascontiguousarray(src_off, np.uint64).view(np.int64)).to(dev)
        d_len = torch.from_numpy(np.ascontiguousarray(src_len, np.uint32).view(np.int32)).to(dev)
        d_dst = torch.from_numpy(dst.view(np.int64)).to(dev)
        # the implementations of one contract: wave None = the default for this launch size, True / False the wave- / the
        # lane-per-block kernel, a string one implementation by name ("lds", "private", "wave", "lane", "fast")
        variant = inflate_variant_for(n) if wave is None else wave if isinstance(wave, str) else ("wave" if wave else "lane")
        launch_inflate(lib, variant, d_comp.data_ptr(), d_src.data_ptr(), d_len.data_ptr(), d_dst.data_ptr(), n, d_out.data_ptr(),
                       d_status.data_ptr(), total, dev)
        if bgzf_crc_wanted() if crc is None else crc:
            # the blocks' footers (CRC32 of the inflated bytes) checked on the device: status 9 where one differs
            rc = lib.svx_bgzf_crc32(d_out.data_ptr(), d_dst.data_ptr(), d_comp.data_ptr(), d_src.data_ptr(), d_len.data_ptr(), n,
                                    d_status.data_ptr(), _stream_ptr(dev))
            _lib.check(rc, "svx_bgzf_crc32")
    return d_out[:total], d_status[:n]


# ---- the records of an unsorted BAM in coordinate order (svx_recsort.hip; the loader: svision_amd/ingest_sort.py) ----
RECORD_SORT_TILE = 2048              # SVX_RECORD_SORT_TILE: records a workgroup of the sort's histogram and scatter passes takes


def _require_order(order, n=None):
    _require_cuda(order, "order")
    if order.dtype != torch.int32 or order.dim() != 1 or (n is not None and order.shape[0] != n):
        raise _lib.SvxError("order must be an int32 [n] tensor (the bits of uint32 indices)")


def record_sort(d_tid, d_pos, n_ref, pos_bits):
    """tid / pos int32 [n] device tensors -> int32 [n] (the bits of uint32): the input index of the record of every sorted rank,
    by (tid, unmapped last; pos), stable.  ``pos_bits``: bit_length(longest reference + 1).  See include/svx.h svx_record_sort."""
    lib = _lib.load()
    _require_cuda(d_tid, "tid")
    _require_cuda(d_pos, "pos")
    if d_tid.dtype != torch.int32 or d_pos.dtype != torch.int32 or d_tid.dim() != 1 or d_tid.shape != d_pos.shape:
        raise _lib.SvxError("tid and pos must be int32 [n] tensors")
    n, dev = int(d_tid.shape[0]), d_tid.device
    order = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.svx_record_sort_ws_bytes(n)), dtype=torch.uint8, device=dev)
    _lib.check(lib.svx_record_sort(d_tid.data_ptr(), d_pos.data_ptr(), n, int(n_ref), int(pos_bits), order.data_ptr(), ws.data_ptr(),
                                   int(ws.numel()), _stream_ptr(dev)), "svx_record_sort")
    return order


def record_gather(src, order):
    """out[r] = src[order[r]] for a 1-D device tensor of 1-, 2- or 4-byte elements.  See include/svx.h svx_record_gather."""
    lib = _lib.load()
    _require_cuda(src, "src")
    _require_order(order)
    if src.dim() != 1 or src.element_size() not in (1, 2, 4):
        raise _lib.SvxError("src must be a 1-D tensor of 1-, 2- or 4-byte elements")
    n = int(order.shape[0])
    out = torch.empty(n, dtype=src.dtype, device=src.device)
    _lib.check(lib.svx_record_gather(src.data_ptr(), order.data_ptr(), out.data_ptr(), n, src.element_size(), _stream_ptr(src.device)),
               "svx_record_gather")
    return out


def record_gather_offsets(off_in, order):
    """off_in int64 [n + 1] (CSR offsets in input order) -> int64 [n + 1]: the offsets of the same segments laid out in the order
    ``order``, the closing entry their total.  See include/svx.h svx_record_gather_offsets."""
    lib = _lib.load()
    _require_cuda(off_in, "off_in")
    n = int(off_in.shape[0]) - 1
    _require_order(order, n)
    if off_in.dtype != torch.int64 or off_in.dim() != 1 or n < 0:
        raise _lib.SvxError("off_in must be an int64 [n + 1] tensor")
    dev = off_in.device
    out = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.svx_record_gather_offsets_ws_bytes(n)), dtype=torch.uint8, device=dev)
    _lib.check(lib.svx_record_gather_offsets(off_in.data_ptr(), order.data_ptr(), n, out.data_ptr(), ws.data_ptr(), int(ws.numel()),
                                             _stream_ptr(dev)), "svx_record_gather_offsets")
    return out


def record_gather_segments(src, off_in, order, off_out, out):
    """Segment ``order[r]`` of ``src`` (elements off_in[s] .. off_in[s + 1]) -> element off_out[r] of ``out`` (same dtype, at least
    off_out[n] elements; nothing else of it is written).  ``src``: readable up to the next multiple of 4 bytes behind its end.
    See include/svx.h svx_record_gather_segments."""
    lib = _lib.load()
    for t, name in ((src, "src"), (off_in, "off_in"), (off_out, "off_out"), (out, "out")):
        _require_cuda(t, name)
    n = int(off_in.shape[0]) - 1
    _require_order(order, n)
    if off_in.dtype != torch.int64 or off_out.dtype != torch.int64 or off_out.shape != off_in.shape or out.dtype != src.dtype \
            or src.element_size() not in (1, 2, 4):
        raise _lib.SvxError("off_in / off_out must be int64 [n + 1], src / out of one dtype of 1, 2 or 4 bytes")
    _lib.check(lib.svx_record_gather_segments(src.data_ptr(), off_in.data_ptr(), order.data_ptr(), off_out.data_ptr(), out.data_ptr(), n,
                                              src.element_size(), _stream_ptr(src.device)), "svx_record_gather_segments")
    return out


def record_invert(order):
    """order int32 [n] (record_sort's) -> int32 [n] (the bits of uint32): rank[order[r]] = r.  See include/svx.h svx_record_invert."""
    lib = _lib.load()
    _require_order(order)
    n = int(order.shape[0])
    rank = torch.empty(n, dtype=torch.int32, device=order.device)
    _lib.check(lib.svx_record_invert(order.data_ptr(), n, rank.data_ptr(), _stream_ptr(order.device)), "svx_record_invert")
    return rank


def record_scatter_segments(src, src_off, rank, rank_lo, rank_hi, off_out, out_base, out, status):
    """The n input records src[src_off[i]:src_off[i + 1]] (uint8; int64 [n + 1]) whose ``rank[i]`` (int32 [n], the bits of uint32) lies
    in [rank_lo, rank_hi) -> ``out`` (uint8) at byte off_out[rank] - out_base; ``off_out``: int64, indexed by rank, at least rank_hi + 1
    entries.  ``status``: int32 [1], set to 1 where a record's length is not off_out's (that record is not copied).  ``src``: 4-byte
    aligned and readable up to the next multiple of 4 bytes behind its end; ``out`` must hold every record of the window whole.
    See include/svx.h svx_record_scatter_segments."""
    lib = _lib.load()
    for t, name in ((src, "src"), (src_off, "src_off"), (off_out, "off_out"), (out, "out"), (status, "status")):
        _require_cuda(t, name)
    n = int(src_off.shape[0]) - 1
    _require_order(rank, n)
    rank_lo, rank_hi = int(rank_lo), int(rank_hi)
    if src_off.dtype != torch.int64 or off_out.dtype != torch.int64 or src.dtype != torch.uint8 or out.dtype != torch.uint8 \
            or status.dtype != torch.int32 or status.numel() < 1:
        raise _lib.SvxError("src_off / off_out must be int64, src / out uint8, status int32 [1]")
    if not 0 <= rank_lo <= rank_hi < int(off_out.shape[0]):
        raise _lib.SvxError("the window [%d, %d) does not lie in off_out's %d ranks" % (rank_lo, rank_hi, int(off_out.shape[0]) - 1))
    _lib.check(lib.svx_record_scatter_segments(src.data_ptr(), src_off.data_ptr(), rank.data_ptr(), rank_lo, rank_hi, off_out.data_ptr(), int(out_base),
                                               out.data_ptr(), n, status.data_ptr(), _stream_ptr(src.device)), "svx_record_scatter_segments")
    return out


def record_retid(d_bytes, d_off, d_map, d_tid_key, status):
    """The n = len(d_off) BAM records that start at d_bytes[d_off[r]] (uint8; int64 [n], any byte offsets): refID (byte 4) and
    next_refID (byte 24) rewritten in place through ``d_map`` (int32 [n_in]) -- -1 stays, 0 <= v < n_in becomes d_map[v] --, and
    ``d_tid_key`` (int32 [n] or None) by the same rule.  ``status``: int32 [1], set to 1 where a field lies outside (that record keeps
    both fields).  Every record needs its first 28 bytes inside ``d_bytes``.  See include/svx.h svx_record_retid."""
    lib = _lib.load()
    for t, name in ((d_bytes, "d_bytes"), (d_off, "d_off"), (d_map, "d_map"), (status, "status")):
        _require_cuda(t, name)
    n = int(d_off.shape[0])
    if d_bytes.dtype != torch.uint8 or d_off.dtype != torch.int64 or d_off.dim() != 1 or d_map.dtype != torch.int32 or d_map.dim() != 1 \
            or status.dtype != torch.int32 or status.numel() < 1:
        raise _lib.SvxError("d_bytes must be uint8, d_off int64 [n], d_map int32 [n_in], status int32 [1]")
    if d_tid_key is not None:
        _require_cuda(d_tid_key, "d_tid_key")
        if d_tid_key.dtype != torch.int32 or d_tid_key.dim() != 1 or d_tid_key.shape[0] != n:
            raise _lib.SvxError("d_tid_key must be int32 [n]")
    if n > 0xFFFFFFFF:
        raise _lib.SvxError("svx_record_retid takes up to 2^32 - 1 records")
    _lib.check(lib.svx_record_retid(d_bytes.data_ptr(), d_off.data_ptr(), n, d_map.data_ptr() if d_map.numel() else None, int(d_map.shape[0]),
                                    None if d_tid_key is None else d_tid_key.data_ptr(), status.data_ptr(), _stream_ptr(d_bytes.device)),
               "svx_record_retid")
    return d_bytes


RetagTable = collections.namedtuple("RetagTable", "d_bytes d_off m")


def retag_pack(renames):
    """{(tag, old): new} -- tag "RG" / "PG" or its bytes, the values bytes -- -> (uint8 bytes, int32 offsets [2m + 1], m) as
    svx_record_retag_measure takes them, on the host: per entry the tag, the old value, the new one, in the mapping's order."""
    flat, off = bytearray(), [0]
    for (tag, old), new in renames.items():
        tag = tag.encode("latin-1") if isinstance(tag, str) else bytes(tag)
        old, new = bytes(old), bytes(new)
        if len(tag) != 2 or b"\0" in old or b"\0" in new:
            raise _lib.SvxError("a rename is a 2-byte tag and two values without NUL: %r" % ((tag, old, new),))
        flat += tag + old
        off.append(len(flat))
        flat += new
        off.append(len(flat))
    if len(flat) > 0x7FFFFFFF:
        raise _lib.SvxError("the renames' bytes exceed 2^31 - 1")
    return np.frombuffer(bytes(flat) or b"\0", np.uint8), np.asarray(off, np.int32), len(renames)


def retag_table(renames, device):
    """:func:`retag_pack` on the device -> RetagTable."""
    flat, off, m = retag_pack(renames)
    return RetagTable(torch.from_numpy(flat.copy()).to(device), torch.from_numpy(off).to(device), m)


def _require_retag(d_bytes, d_off, table, status):
    for t, name in ((d_bytes, "d_bytes"), (d_off, "d_off"), (table.d_bytes, "table.d_bytes"), (table.d_off, "table.d_off"), (status, "status")):
        _require_cuda(t, name)
    if d_bytes.dtype != torch.uint8 or d_off.dtype != torch.int64 or d_off.dim() != 1 or d_off.shape[0] < 1 or status.dtype != torch.int32 \
            or status.numel() < 1:
        raise _lib.SvxError("d_bytes must be uint8, d_off int64 [n + 1], status int32 [1]")
    if table.d_bytes.dtype != torch.uint8 or table.d_off.dtype != torch.int32 or table.d_off.dim() != 1 or table.d_off.shape[0] != 2 * table.m + 1:
        raise _lib.SvxError("a table is uint8 bytes and int32 offsets [2m + 1]")
    n = int(d_off.shape[0]) - 1
    if n > 0xFFFFFFFF:
        raise _lib.SvxError("svx_record_retag takes up to 2^32 - 1 records")
    return n


def record_retag_measure(d_bytes, d_off, table, status):
    """The n BAM records d_bytes[d_off[r]:d_off[r + 1]] (uint8; int64 [n + 1], any byte offsets) -> int64 [n]: every record's length
    once the first RG:Z and the first PG:Z value that ``table`` (:func:`retag_table`) renames are replaced.  ``status``: int32 [1],
    set to 1 where a record is malformed (it keeps its length).  An empty table: the lengths as they are, no launch.
    See include/svx.h svx_record_retag_measure."""
    lib = _lib.load()
    n = _require_retag(d_bytes, d_off, table, status)
    if table.m == 0:
        return d_off[1:] - d_off[:-1]
    d_new_len = torch.empty(n, dtype=torch.int64, device=d_bytes.device)
    _lib.check(lib.svx_record_retag_measure(d_bytes.data_ptr(), d_off.data_ptr(), n, table.d_bytes.data_ptr(), table.d_off.data_ptr(), table.m,
                                            d_new_len.data_ptr(), status.data_ptr(), _stream_ptr(d_bytes.device)), "svx_record_retag_measure")
    return d_new_len


def record_retag_write(d_bytes, d_off, table, d_new_off, out, status):
    """The records of :func:`record_retag_measure` rewritten -> ``out`` (uint8), record r at byte d_new_off[r] (int64 [n + 1], the
    exclusive sum of measure's lengths; ``out`` holds at least d_new_off[n] bytes, nothing else of it is written), block_size set.
    ``status``: set to 1 where a record is malformed (copied as it is) or d_new_off gives it another length than measure (not
    copied).  ``d_bytes``: readable up to the next multiple of 4 bytes behind its end.  See include/svx.h svx_record_retag_write."""
    lib = _lib.load()
    n = _require_retag(d_bytes, d_off, table, status)
    for t, name in ((d_new_off, "d_new_off"), (out, "out")):
        _require_cuda(t, name)
    if d_new_off.dtype != torch.int64 or d_new_off.shape != d_off.shape or out.dtype != torch.uint8 or out.dim() != 1:
        raise _lib.SvxError("d_new_off must be int64 [n + 1], out uint8")
    if table.m == 0:
        raise _lib.SvxError("svx_record_retag_write: an empty table rewrites nothing")
    _lib.check(lib.svx_record_retag_write(d_bytes.data_ptr(), d_off.data_ptr(), n, table.d_bytes.data_ptr(), table.d_off.data_ptr(), table.m,
                                          d_new_off.data_ptr(), out.data_ptr(), status.data_ptr(), _stream_ptr(d_bytes.device)),
               "svx_record_retag_write")
    return out


TAGS_TABLE_BYTES = 8192             # SVX_RECORD_TAGS_TABLE_BYTES: a bit for every two-byte tag value
TAGS_ALWAYS_KEPT = ("CG",)          # the real CIGAR of a record with more than 65,535 operations: never removed


def tags_bitmap(tags, keep):
    """``tags``: 2-character tags (str or bytes) -> the table of svx_record_tags_measure on the host, int32 [2048]: bit
    (t0 | t1 << 8) set = a field of that tag is removed.  ``keep`` unset: the listed tags are removed; set: every tag BUT the listed
    ones -- an empty list removes all.  ``CG`` is never removed: naming it in a drop list is an error, a keep list implies it."""
    keys = []
    for tag in tuple(tags) + (TAGS_ALWAYS_KEPT if keep else ()):
        raw = tag.encode("latin-1") if isinstance(tag, str) else bytes(tag)
        if len(raw) != 2:
            raise _lib.SvxError("a tag is two bytes: %r" % (tag,))
        if not keep and raw.decode("latin-1") in TAGS_ALWAYS_KEPT:
            raise _lib.SvxError("%s is never removed" % raw.decode("latin-1"))
        keys.append(raw[0] | raw[1] << 8)
    bits = np.full(TAGS_TABLE_BYTES, 0xFF if keep else 0, np.uint8)
    for k in keys:
        if keep:
            bits[k >> 3] &= 0xFF ^ (1 << (k & 7))
        else:
            bits[k >> 3] |= 1 << (k & 7)
    return bits.view("<i4")


def tags_table(tags, keep, device):
    """:func:`tags_bitmap` on the device -> int32 [2048], what :func:`record_tags_measure` and :func:`record_tags_write` take."""
    return torch.from_numpy(tags_bitmap(tags, keep).copy()).to(device)


def _require_tags(d_bytes, d_off, table, status):
    for t, name in ((d_bytes, "d_bytes"), (d_off, "d_off"), (table, "table"), (status, "status")):
        _require_cuda(t, name)
    if d_bytes.dtype != torch.uint8 or d_off.dtype != torch.int64 or d_off.dim() != 1 or d_off.shape[0] < 1 or status.dtype != torch.int32 \
            or status.numel() < 1:
        raise _lib.SvxError("d_bytes must be uint8, d_off int64 [n + 1], status int32 [1]")
    if table.dtype != torch.int32 or table.dim() != 1 or table.shape[0] * 4 != TAGS_TABLE_BYTES or not table.is_contiguous():
        raise _lib.SvxError("a tags table is int32 [%d], contiguous (tags_table)" % (TAGS_TABLE_BYTES // 4))
    n = int(d_off.shape[0]) - 1
    if n > 0xFFFFFFFF:
        raise _lib.SvxError("svx_record_tags takes up to 2^32 - 1 records")
    return n


def record_tags_measure(d_bytes, d_off, table, status):
    """The n BAM records d_bytes[d_off[r]:d_off[r + 1]] (uint8; int64 [n + 1], any byte offsets) -> int64 [n]: every record's length
    without the optional fields that ``table`` (:func:`tags_table`) removes.  ``status``: int32 [1], set to 1 where a record is
    malformed (it keeps its length).  See include/svx.h svx_record_tags_measure."""
    lib = _lib.load()
    n = _require_tags(d_bytes, d_off, table, status)
    d_new_len = torch.empty(n, dtype=torch.int64, device=d_bytes.device)
    _lib.check(lib.svx_record_tags_measure(d_bytes.data_ptr(), d_off.data_ptr(), n, table.data_ptr(), d_new_len.data_ptr(), status.data_ptr(),
                                           _stream_ptr(d_bytes.device)), "svx_record_tags_measure")
    return d_new_len


def record_tags_write(d_bytes, d_off, table, d_new_off, out, status):
    """The records of :func:`record_tags_measure` without those fields -> ``out`` (uint8), record r at byte d_new_off[r] (int64
    [n + 1], the exclusive sum of measure's lengths; ``out`` holds at least d_new_off[n] bytes, nothing else of it is written),
    block_size set.  ``status``: set to 1 where a record is malformed (copied as it is) or d_new_off gives it another length than
    measure (not copied).  ``d_bytes``: readable up to the next multiple of 4 bytes behind its end.  See include/svx.h
    svx_record_tags_write."""
    lib = _lib.load()
    n = _require_tags(d_bytes, d_off, table, status)
    for t, name in ((d_new_off, "d_new_off"), (out, "out")):
        _require_cuda(t, name)
    if d_new_off.dtype != torch.int64 or d_new_off.shape != d_off.shape or out.dtype != torch.uint8 or out.dim() != 1:
        raise _lib.SvxError("d_new_off must be int64 [n + 1], out uint8")
    _lib.check(lib.svx_record_tags_write(d_bytes.data_ptr(), d_off.data_ptr(), n, table.data_ptr(), d_new_off.data_ptr(), out.data_ptr(),
                                         status.data_ptr(), _stream_ptr(d_bytes.device)), "svx_record_tags_write")
    return out


# ---- BGZF members from inflated bytes (svx_deflate.hip; the writer: svision_amd/sort.py) ----
BGZF_SLOT = 65536                    # SVX_BGZF_SLOT: bytes of a member's slot in svx_bgzf_deflate's output
BGZF_BLOCK_MAX = 0xFF00              # SVX_BGZF_BLOCK_MAX: the largest block the encoder takes (htslib's block size)
BGZF_MEMBER_EXTRA = 31               # a member is never longer than its block + header 18 + stored 5 + footer 8


def bgzf_deflate(d_in, d_in_off):
    """d_in: uint8 device tensor, d_in_off: int64 [n + 1] device tensor -- block b = d_in[d_in_off[b]:d_in_off[b + 1]], 0 .. 0xFF00
    bytes, any alignment -> (uint8 [n, 65536] slots, int32 [n] member lengths, int32 [n] 1 where the block is stored).  Fixed
    Huffman code or stored, whichever is smaller; the bytes are a pure function of the input.  See include/svx.h svx_bgzf_deflate."""
    lib = _lib.load()
    _require_cuda(d_in, "d_in")
    _require_cuda(d_in_off, "d_in_off")
    if d_in.dtype != torch.uint8 or d_in_off.dtype != torch.int64 or d_in_off.dim() != 1 or d_in_off.shape[0] < 1:
        raise _lib.SvxError("d_in must be uint8, d_in_off int64 [n + 1]")
    n, dev = int(d_in_off.shape[0]) - 1, d_in.device
    slots = torch.empty((n, BGZF_SLOT), dtype=torch.uint8, device=dev)
    member_len = torch.zeros(n, dtype=torch.int32, device=dev)
    stored = torch.zeros(n, dtype=torch.int32, device=dev)
    _lib.check(lib.svx_bgzf_deflate(d_in.data_ptr(), d_in_off.data_ptr(), n, slots.data_ptr(), member_len.data_ptr(), stored.data_ptr(),
                                    _stream_ptr(dev)), "svx_bgzf_deflate")
    return slots, member_len, stored


def bgzf_deflate_dynamic(d_in, d_in_off, phase_ticks=False):
    """:func:`bgzf_deflate` with dynamic Huffman tables as a third form -> (uint8 [n, 65536] slots, int32 [n] member lengths, int32 [n]
    block types: 0 stored, 1 fixed code, 2 dynamic codes -- the smallest of the three, stored at a tie, then fixed).  The same parse:
    where the type is 0 or 1 the member is :func:`bgzf_deflate`'s, byte for byte.  :func:`bgzf_pack` takes the output as it is.
    ``phase_ticks``: also return int64 [n, 4], the device's 100 MHz clock at each block's start, after its parse, after its code
    construction and at its end.  See include/svx.h svx_bgzf_deflate_dyn."""
    lib = _lib.load()
    _require_cuda(d_in, "d_in")
    _require_cuda(d_in_off, "d_in_off")
    if d_in.dtype != torch.uint8 or d_in_off.dtype != torch.int64 or d_in_off.dim() != 1 or d_in_off.shape[0] < 1:
        raise _lib.SvxError("d_in must be uint8, d_in_off int64 [n + 1]")
    n, dev = int(d_in_off.shape[0]) - 1, d_in.device
    slots = torch.empty((n, BGZF_SLOT), dtype=torch.uint8, device=dev)
    member_len = torch.zeros(n, dtype=torch.int32, device=dev)
    btype = torch.zeros(n, dtype=torch.int32, device=dev)
    need = int(lib.svx_bgzf_deflate_dyn_ws_bytes(n))
    ws = torch.empty(max(need + (32 * n if phase_ticks else 0), 8), dtype=torch.uint8, device=dev)
    if phase_ticks:
        ws[need:] = 0
    _lib.check(lib.svx_bgzf_deflate_dyn(d_in.data_ptr(), d_in_off.data_ptr(), n, slots.data_ptr(), member_len.data_ptr(), btype.data_ptr(),
                                        ws.data_ptr(), int(ws.numel()) if n else 0, _stream_ptr(dev)), "svx_bgzf_deflate_dyn")
    if phase_ticks:
        return slots, member_len, btype, ws[need:need + 32 * n].view(torch.int64).view(n, 4).clone()
    return slots, member_len, btype


def bgzf_pack(slots, member_len, out_bytes):
    """The members of :func:`bgzf_deflate` end to end -> (uint8 [out_bytes] device tensor whose first file_off[n] bytes are the file
    bytes, int64 [n + 1] device tensor file_off: the exclusive prefix sum of the lengths, taken on the device).  ``out_bytes``: at
    least the blocks' bytes + 31 a block.  See include/svx.h svx_bgzf_pack."""
    lib = _lib.load()
    _require_cuda(slots, "slots")
    _require_cuda(member_len, "member_len")
    n, dev = int(member_len.shape[0]), slots.device
    if slots.dtype != torch.uint8 or member_len.dtype != torch.int32 or slots.numel() != n * BGZF_SLOT:
        raise _lib.SvxError("slots must be uint8 [n, 65536], member_len int32 [n]")
    out = torch.empty(max(int(out_bytes), 1), dtype=torch.uint8, device=dev)
    file_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    _lib.check(lib.svx_bgzf_pack(slots.data_ptr(), member_len.data_ptr(), n, file_off.data_ptr(), out.data_ptr(), int(out_bytes), _stream_ptr(dev)),
               "svx_bgzf_pack")
    return out, file_off


# ---- SAM text -> BAM records (svx_sam.hip; the rules: svision_amd/io/sam.py; the caller: svision_amd/sort.py) ----
SAM_SLACK = 64                       # SVX_SAM_SLACK: readable bytes behind a chunk of text
SAM_HOST = -1                        # SVX_SAM_HOST: a valid line the kernels leave to svision_amd.io.sam.encode_line

SamRefTable = collections.namedtuple("SamRefTable", "hash tid name_off names n")


def sam_ref_table(references, device):
    """The @SQ names (str, in tid order) -> the device table the SAM kernels look RNAME and RNEXT up in: the names' FNV-1a hashes
    ascending, their tids in that order, and the names' bytes by tid (the kernels compare them)."""
    from .io.sam import name_hash
    names = [r.encode("latin-1") for r in references]
    hashes = np.fromiter((name_hash(n) for n in names), np.uint32, len(names))
    by_hash = np.argsort(hashes, kind="stable").astype(np.int32)
    name_off = np.zeros(len(names) + 1, np.uint32)
    name_off[1:] = np.cumsum([len(n) for n in names], dtype=np.int64)
    flat = np.frombuffer(b"".join(names) or b"\0", np.uint8)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype).copy()).to(device)
    return SamRefTable(to(hashes[by_hash]), to(by_hash), to(name_off), to(flat), len(names))


def _require_text(d_text, n_bytes):
    _require_cuda(d_text, "d_text")
    if d_text.dtype != torch.uint8 or d_text.numel() < int(n_bytes) + SAM_SLACK:
        raise _lib.SvxError("d_text must be uint8 with %d readable bytes behind the chunk's %d" % (SAM_SLACK, n_bytes))


class SamLinesOverflow(_lib.SvxError):
    def __init__(self, n_lines, cap):
        _lib.SvxError.__init__(self, "svx_sam_lines: %d lines, the table holds %d" % (n_lines, cap - 1))
        self.n_lines = n_lines


def sam_lines(d_text, n_bytes, cap=None):
    """The chunk d_text[:n_bytes] of alignment lines (SAM_SLACK readable bytes behind it) -> (int64 [cap] device tensor whose first
    n_lines + 1 entries are the line starts and n_bytes, n_lines).  ``cap``: at least the chunk's lines + 1; None: a call that only
    counts comes first.  See include/svx.h svx_sam_lines."""
    lib = _lib.load()
    _require_text(d_text, n_bytes)
    if cap is None:
        try:
            return sam_lines(d_text, n_bytes, 1)
        except SamLinesOverflow as exc:
            return sam_lines(d_text, n_bytes, exc.n_lines + 1)
    dev, cap = d_text.device, max(int(cap), 1)
    line_off = torch.empty(cap, dtype=torch.int64, device=dev)
    n_lines = torch.zeros(1, dtype=torch.int64, device=dev)
    ws_bytes = int(lib.svx_sam_lines_ws_bytes(int(n_bytes)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.svx_sam_lines(d_text.data_ptr(), int(n_bytes), line_off.data_ptr(), cap, n_lines.data_ptr(), ws.data_ptr(), ws_bytes,
                                 _stream_ptr(dev)), "svx_sam_lines")
    n = int(n_lines.item())
    if n + 1 > cap:
        raise SamLinesOverflow(n, cap)
    return line_off, n


def sam_measure(d_text, n_bytes, line_off, n_lines, table):
    """A wave a line -> int32 [n_lines] device tensors (len, tid, pos, flag, span): the bytes of the line's BAM record or a negative
    code (SAM_HOST, or an error: svision_amd.io.sam.E_*), and the sort key and index fields.  See include/svx.h svx_sam_measure."""
    lib = _lib.load()
    _require_text(d_text, n_bytes)
    dev = d_text.device
    if line_off.dtype != torch.int64 or line_off.numel() < n_lines + 1 or n_lines > 0xFFFFFFFF:
        raise _lib.SvxError("line_off must be int64 [n_lines + 1]")
    out = [torch.empty(n_lines, dtype=torch.int32, device=dev) for _ in range(5)]
    _lib.check(lib.svx_sam_measure(d_text.data_ptr(), line_off.data_ptr(), n_lines, table.hash.data_ptr(), table.tid.data_ptr(),
                                   table.name_off.data_ptr(), table.names.data_ptr(), table.n, *[t.data_ptr() for t in out], _stream_ptr(dev)),
               "svx_sam_measure")
    return tuple(out)


def sam_encode(d_text, n_bytes, line_off, n_lines, table, d_len, d_off, out_base, out, status):
    """A wave a line: the record of every line with ``d_len[i] >= 0`` (int32 [n_lines]) to ``out`` (uint8) at byte d_off[i] - out_base
    (int64 [n_lines]), exactly d_len[i] bytes; ``out`` must hold them all, which is checked here.  ``status``: int32 [1], set to 1 where a line no longer measures d_len[i] --
    that record is not written.  See include/svx.h svx_sam_encode."""
    lib = _lib.load()
    _require_text(d_text, n_bytes)
    for t, name in ((d_len, "d_len"), (d_off, "d_off"), (out, "out"), (status, "status")):
        _require_cuda(t, name)
    if d_len.dtype != torch.int32 or d_off.dtype != torch.int64 or out.dtype != torch.uint8 or status.dtype != torch.int32 \
            or d_len.numel() < n_lines or d_off.numel() < n_lines or line_off.numel() < n_lines + 1:
        raise _lib.SvxError("d_len must be int32 [n_lines], d_off int64 [n_lines], out uint8, status int32 [1]")
    if n_lines:
        ends = (d_off[:n_lines] + d_len[:n_lines].clamp(min=0)) - int(out_base)
        taken = d_len[:n_lines] >= 0
        if bool(taken.any()) and (int(ends[taken].max()) > out.numel() or int((d_off[:n_lines][taken] - int(out_base)).min()) < 0):
            raise _lib.SvxError("svx_sam_encode: a record lies outside the %d bytes of out" % out.numel())
    _lib.check(lib.svx_sam_encode(d_text.data_ptr(), line_off.data_ptr(), n_lines, table.hash.data_ptr(), table.tid.data_ptr(),
                                  table.name_off.data_ptr(), table.names.data_ptr(), table.n, d_len.data_ptr(), d_off.data_ptr(), int(out_base),
                                  out.data_ptr(), status.data_ptr(), _stream_ptr(d_text.device)), "svx_sam_encode")
    return out


# ---- SAM text -> the device ingest's packed arrays (svx_sam.hip; the caller: svision_amd/ingest_sort.py) ----
def sam_pack_count(d_text, n_bytes, line_off, n_lines, table, with_seq=False):
    """A wave a line -> (status int32 [n_lines], fields int32 [5, n_lines]: tid pos flag mapq l_seq, counts int32 [3, n_lines]: CIGAR
    words, name bytes, SEQ bytes) on the device.  status: 0, SAM_HOST (a ``<l_seq>S<n>N`` CIGAR: the caller's), or an error code
    (svision_amd.io.sam.E_*).  See include/svx.h svx_sam_pack_count."""
    lib = _lib.load()
    _require_text(d_text, n_bytes)
    dev = d_text.device
    if line_off.dtype != torch.int64 or line_off.numel() < n_lines + 1 or n_lines > 0xFFFFFFFF:
        raise _lib.SvxError("line_off must be int64 [n_lines + 1]")
    status = torch.empty(n_lines, dtype=torch.int32, device=dev)
    fields, counts = torch.empty((5, n_lines), dtype=torch.int32, device=dev), torch.empty((3, n_lines), dtype=torch.int32, device=dev)
    _lib.check(lib.svx_sam_pack_count(d_text.data_ptr(), line_off.data_ptr(), n_lines, table.hash.data_ptr(), table.tid.data_ptr(),
                                      table.name_off.data_ptr(), table.names.data_ptr(), table.n, int(bool(with_seq)), status.data_ptr(),
                                      fields.data_ptr(), counts.data_ptr(), _stream_ptr(dev)), "svx_sam_pack_count")
    return status, fields, counts


def sam_pack_extract(d_text, n_bytes, line_off, n_lines, table, status, offsets, out):
    """A wave a line: every line with ``status[i] == 0`` into the packed arrays ``out`` -- a dict of device tensors d_tid d_pos d_l_seq
    (int32 [n_lines]), d_flag (int16), d_mapq (uint8), d_cigar (int32), d_names (uint8) and, for the bases, d_seq (uint8).
    ``offsets``: host int64 arrays [n_lines + 1] (cigar, names and, with d_seq, seq), the exclusive prefix of sam_pack_count's counts;
    they must ascend and end inside their array, which is checked here.  -> the offsets on the device, in that order.  See
    include/svx.h svx_sam_pack_extract."""
    lib = _lib.load()
    _require_text(d_text, n_bytes)
    dev = d_text.device
    with_seq = out.get("d_seq") is not None
    want = (("d_tid", torch.int32), ("d_pos", torch.int32), ("d_l_seq", torch.int32), ("d_flag", torch.int16), ("d_mapq", torch.uint8))
    for name, dtype in want:
        _require_cuda(out[name], name)
        if out[name].dtype != dtype or out[name].numel() < n_lines:
            raise _lib.SvxError("%s must be %s [n_lines]" % (name, dtype))
    data = [("d_cigar", torch.int32), ("d_names", torch.uint8)] + ([("d_seq", torch.uint8)] if with_seq else [])
    if len(offsets) != len(data) or status.dtype != torch.int32 or status.numel() < n_lines or line_off.numel() < n_lines + 1:
        raise _lib.SvxError("status must be int32 [n_lines], and one offsets array per data array")
    d_off = []
    for (name, dtype), off in zip(data, offsets):
        _require_cuda(out[name], name)
        off = np.ascontiguousarray(off, np.int64)
        if out[name].dtype != dtype or off.size != n_lines + 1 or int(off[0]) < 0 or (np.diff(off) < 0).any() or int(off[-1]) > out[name].numel():
            raise _lib.SvxError("svx_sam_pack_extract: the offsets of %s do not ascend inside its %d elements" % (name, out[name].numel()))
        d_off.append(torch.from_numpy(off).to(dev))
    spare = torch.empty(4, dtype=torch.uint8, device=dev)      # (an array of no element has no address: nothing is written there)
    ptr = lambda t: t.data_ptr() if t.numel() else spare.data_ptr()
    seq = (d_off[2].data_ptr(), ptr(out["d_seq"])) if with_seq else (None, None)
    _lib.check(lib.svx_sam_pack_extract(d_text.data_ptr(), line_off.data_ptr(), n_lines, table.hash.data_ptr(), table.tid.data_ptr(),
                                        table.name_off.data_ptr(), table.names.data_ptr(), table.n, status.data_ptr(), out["d_tid"].data_ptr(),
                                        out["d_pos"].data_ptr(), out["d_flag"].data_ptr(), out["d_mapq"].data_ptr(), out["d_l_seq"].data_ptr(),
                                        d_off[0].data_ptr(), ptr(out["d_cigar"]), d_off[1].data_ptr(), ptr(out["d_names"]),
                                        seq[0], seq[1], _stream_ptr(dev)), "svx_sam_pack_extract")
    return d_off
