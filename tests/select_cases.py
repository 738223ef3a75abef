"""Cases and the NumPy reference of the top-scale selection rule (csrc/sift_select.h), shared by the
CPU test of sgsel::select_host (tests/test_select.py) and the GPU test of k_select_top_scale
(tests/test_gpu_prematch.py).  The expected values come from NumPy alone: a stable argsort of the
negated order key, cut at `top`, sorted back into index order."""
from __future__ import annotations

import numpy as np

SIZES = [0, 1, 63, 64, 65, 99, 100, 101, 255, 256, 257, 1000, 5000]
TOPS = [1, 7, 64, 100, 6000]
PATTERNS = ["random", "equal", "three", "ascending", "descending", "byte0", "byte1", "byte2", "byte3"]


def order_key(scale: np.ndarray) -> np.ndarray:
    """sgsel::order_key on the float32 bits: sign set -> ~bits, else bits | 0x80000000."""
    bits = np.ascontiguousarray(scale, np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def numpy_select(scale: np.ndarray, top: int) -> np.ndarray:
    key = order_key(scale).astype(np.int64)
    return np.sort(np.argsort(-key, kind="stable")[:top]).astype(np.int32)


def _three(n, top, rng):
    """Three distinct values; where n > top the middle group straddles the cut: g rows above it,
    quota = top - g of the group's rows taken, at least one and not all of them."""
    if n <= top:
        return rng.choice(np.array([1.5, 2.5, 3.5], np.float32), n)
    g = top // 2
    quota = top - g
    mid = quota + max(1, (n - top) // 2)
    v = np.concatenate([np.full(g, 3.5), np.full(mid, 2.5), np.full(n - g - mid, 1.5)]).astype(np.float32)
    assert len(v) == n and 0 < quota < mid
    return rng.permutation(v)


def pattern(name: str, n: int, top: int, seed: int) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(seed))
    if name == "random":
        return rng.uniform(0.5, 40.0, n).astype(np.float32)
    if name == "equal":
        return np.full(n, 2.0, np.float32)
    if name == "three":
        return _three(n, top, rng)
    if name == "ascending":
        return (np.arange(n, dtype=np.float32) + 1) * np.float32(0.25)
    if name == "descending":
        return (np.arange(n, 0, -1).astype(np.float32)) * np.float32(0.25)
    # keys that differ in one byte only, so that one radix pass decides alone (positive, finite;
    # few values, so ties too)
    b = int(name[-1])
    hi = 0x7F if b == 3 else 0x100
    base = np.uint32(0x40345678) & ~np.uint32(0xFF << (8 * b))
    byte = rng.integers(1 if b == 3 else 0, hi, n).astype(np.uint32)
    return (base | (byte << np.uint32(8 * b))).astype(np.uint32).view(np.float32)


def caller_data(seed: int = 77) -> np.ndarray:
    """What no extraction produces: -0.0, negatives, both infinities, NaNs of both signs, among
    ordinary values.  The rule orders them by order_key, without special cases."""
    rng = np.random.Generator(np.random.PCG64(seed))
    special = np.array([-0.0, 0.0, -1.0, -3.5, np.inf, -np.inf, np.nan, 1e-42, -1e-42], np.float32)
    neg_nan = np.array([0xFFC00001], np.uint32).view(np.float32)
    v = np.concatenate([special, neg_nan, special[:4], rng.uniform(-5, 5, 23).astype(np.float32)])
    return rng.permutation(v)


def sets_for(top: int):
    """[(label, scales)] for one value of top: every pattern at every size, and the caller-data set."""
    out = []
    for pi, name in enumerate(PATTERNS):
        for n in SIZES:
            out.append((f"{name} n={n}", pattern(name, n, top, 9000 + 100 * pi + n % 97)))
    out.append(("caller data", caller_data()))
    return out


def strided(flat: np.ndarray, stride: int, column: int = 0) -> np.ndarray:
    """The scales as column `column` of a [rows][stride] buffer of other values; returns the flat
    view that starts at the first scale (so row r's scale is element r * stride)."""
    buf = np.full((max(len(flat), 1), stride), -123.0, np.float32)
    buf[:len(flat), column] = flat
    return buf.reshape(-1)[column:]
