"""Crafted record streams for svx_record_retid (svision_amd/csrc/svx_recsort_core.hpp: retid_record) and their expected translation,
shared by tests/test_sort_merge_cpu.py (the host program under sanitizers) and tests/test_gpu_record_retid.py (the kernel).

Test-side only: ``struct`` and NumPy.  A stream is ``skew`` sentinel bytes and then n records of 36 .. 200 bytes end to end, the last
one ending with the buffer.  A record: block_size (its length - 4) at byte 0, refID at byte 4, next_refID at byte 24, every other
byte a seeded pseudo-random value -- the routine may touch none of them, and the expectation is the input with the two fields
rewritten by ``struct.pack_into``, so every such byte is compared."""
import struct
import subprocess

import numpy as np

INT32_MIN = -(1 << 31)
SIZES = (0, 1, 2, 65, 300)


def table(n_in, seed=0, spread=5):
    """An injective table of ``n_in`` entries into a dictionary of n_in + spread references."""
    return np.random.default_rng(100 + seed).permutation(n_in + spread)[:n_in].astype(np.int32)


def stream(n, skew, n_in, seed=0, bad=False):
    """-> (bytes uint8, off int64 [n], key int32 [n]).  Fields cycle through -1, 0, n_in - 1 and random values inside; ``bad``: some
    records carry n_in or INT32_MIN in one of the two fields, and one sound record carries a key that is outside."""
    rng = np.random.default_rng(seed * 1000 + n * 4 + skew)
    lens = rng.integers(36, 200, n, endpoint=True)
    if n > 1:
        lens[0], lens[-1] = 36, 36                              # the shortest record at both ends: nothing behind byte 36 of the last
    off = (skew + np.concatenate([[0], np.cumsum(lens)[:-1]])).astype(np.int64) if n else np.zeros(0, np.int64)
    data = bytearray(rng.integers(0, 256, skew + int(lens.sum()), dtype=np.uint8).tobytes())
    inside = [-1, 0, n_in - 1] if n_in else [-1]
    key = np.zeros(n, np.int32)
    for r in range(n):
        tid = inside[r % len(inside)] if r % 4 else (int(rng.integers(0, n_in)) if n_in else -1)
        nxt = inside[(r // 3) % len(inside)] if r % 5 else (int(rng.integers(0, n_in)) if n_in else -1)
        if bad and r % 7 == 1:
            tid = (n_in, INT32_MIN)[(r // 7) % 2]
        if bad and r % 11 == 3:
            nxt = (INT32_MIN, n_in, -2)[(r // 11) % 3]
        struct.pack_into("<iiiiiii", data, int(off[r]), int(lens[r]) - 4, tid, *(int(v) for v in rng.integers(INT32_MIN, 1 << 31, 4)), nxt)
        key[r] = tid
    if bad and n > 2 and 0 <= struct.unpack_from("<i", data, int(off[2]) + 4)[0] < max(n_in, 1):
        key[2] = n_in + 3                                       # a key outside beside a record that is sound
    return np.frombuffer(bytes(data), np.uint8).copy(), off, key


def translate(v, table_):
    """-> (the value the field takes, whether it is inside)."""
    if v == -1:
        return -1, True
    if 0 <= v < len(table_):
        return int(table_[v]), True
    return v, False


def expected(data, off, table_, key=None):
    """The stream after the launch -> (bytes, key or None, status), by struct.pack_into on a copy."""
    out, status = bytearray(data.tobytes()), 0
    new_key = None if key is None else key.copy()
    for r, at in enumerate(int(v) for v in off):
        (tid, ok_t), (nxt, ok_n) = translate(struct.unpack_from("<i", out, at + 4)[0], table_), translate(struct.unpack_from("<i", out, at + 24)[0], table_)
        if ok_t and ok_n:
            struct.pack_into("<i", out, at + 4, tid)
            struct.pack_into("<i", out, at + 24, nxt)
        else:
            status = 1
        if key is not None:
            k, ok = translate(int(key[r]), table_)
            new_key[r] = k
            status |= not ok
    return np.frombuffer(bytes(out), np.uint8).copy(), new_key, int(status)


def run_host(program, path, data, off, table_, key=None):
    """The stand-alone host program on the stream -> (bytes, key or None, status) as it left them."""
    n = len(off)
    with open(path, "wb") as f:
        f.write(np.asarray([n, len(table_), data.size, key is not None], np.int64).tobytes() + off.astype(np.int64).tobytes()
                + np.asarray(table_, np.int32).tobytes() + (b"" if key is None else key.astype(np.int32).tobytes()) + data.tobytes())
    r = subprocess.run([program, path, path + ".out"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = open(path + ".out", "rb").read()
    status = struct.unpack_from("<i", raw, 0)[0]
    new_key = None if key is None else np.frombuffer(raw, np.int32, n, 4).copy()
    at = 4 + (0 if key is None else 4 * n)
    assert len(raw) == at + data.size
    return np.frombuffer(raw, np.uint8, data.size, at).copy(), new_key, status
