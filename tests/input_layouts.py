"""Caller-side input layouts for the extract tests: images whose rows are `stride` elements apart,
with every padding element poisoned, and the list of layouts test_gpu_input_layout.py runs (the
CPU test test_input_layouts.py checks that each of them can show a wrong pitch or a wrong clamp).

stride counts elements for gray u8 / f32 input and bytes for colour, as include/sgpu.h defines it;
image i starts i * stride * h elements into the buffer."""
from __future__ import annotations

import numpy as np

# (n, w, h), the smallest shapes that reach each ingest path
SHAPES = {
    "A": (3, 203, 97),   # ragged width; three images so that a two-part split is 2 + 1
    "B": (2, 482, 40),   # level width 480: the cooperative paired-level kernel's one-strip fit
    "C": (2, 16, 16),    # both edges inside one quad row
}
SEEDS = {"A": 310, "B": 320, "C": 330}

# u8 layouts (shape, stride, byte offset of the device base; offsets != 0 are device input only)
U8_LAYOUTS = [
    ("A", 203, 0),    # control: rows w apart
    ("A", 204, 0),    # stride * h % 16 == 12: images and parts differ in 16-byte alignment
    ("A", 205, 0),    # stride % 4 == 1: nothing may vectorise
    ("A", 208, 0),    # ragged width, aligned pitch: everything may vectorise
    ("A", 256, 0),    # pitch far wider than the row
    ("A", 208, 1),    # no vector form allowed
    ("A", 208, 4),    # the tile and paired kernels may vectorise, the wave kernel may not
    ("A", 208, 16),   # as aligned
    ("B", 482, 0), ("B", 483, 0), ("B", 484, 0), ("B", 512, 0),
    ("C", 16, 0), ("C", 17, 0), ("C", 20, 0), ("C", 64, 0),
]
# f32 (shape A; stride in floats, offset in bytes)
F32_LAYOUTS = [("A", s, o) for s in (203, 204, 205, 208) for o in (0, 4, 16)]
# colour (shape A's first two images; stride in bytes): (format, stride)
COLOR_LAYOUTS = [("rgb", 609), ("rgb", 612), ("rgb", 640), ("bgra", 812), ("bgra", 816),
                 ("bgra", 1024)]
COLOR_OFFSETS = (1, 3)


_IMAGES = {}


def images(shape: str) -> np.ndarray:
    """The dense u8 images [n, h, w] of a shape of SHAPES (generated once, read-only)."""
    if shape not in _IMAGES:
        from sift_synth import synth_batch
        n, w, h = SHAPES[shape]
        a = synth_batch(n, w, h, SEEDS[shape])
        a.setflags(write=False)
        _IMAGES[shape] = a
    return _IMAGES[shape]


def color_images(fmt: str) -> np.ndarray:
    """Shape A's first two images as colour [2, h, w, 3 | 4]: per-channel noise on the gray."""
    key = ("color", fmt)
    if key not in _IMAGES:
        n, w, h = SHAPES["A"]
        ch = 3 if fmt in ("rgb", "bgr") else 4
        rng = np.random.default_rng(5)
        base = images("A")[:2].astype(np.int32)
        a = np.clip(base[..., None] + rng.integers(-40, 41, (2, h, w, ch)), 0, 255).astype(np.uint8)
        a.setflags(write=False)
        _IMAGES[key] = a
    return _IMAGES[key]


def row_elems(images: np.ndarray) -> int:
    """Elements of one dense row: w, or w * c for [n, h, w, c]."""
    return int(np.prod(images.shape[2:]))


def poison(dtype, rows: int, cols: int, col0: int) -> np.ndarray:
    """[rows, cols] of poison for columns col0 .. col0 + cols - 1: u8 0 / 255 by the parity of
    row + column, f32 NaN."""
    if np.dtype(dtype) == np.float32:
        return np.full((rows, cols), np.nan, np.float32)
    r = np.arange(rows)[:, None]
    c = np.arange(col0, col0 + cols)[None, :]
    return (((r + c) & 1) * 255).astype(np.uint8)


def pad(images: np.ndarray, stride: int, poisoned: bool = True) -> np.ndarray:
    """The flat buffer of [n, h, w(, c)] images with rows `stride` elements apart and images
    stride * h apart; every padding element holds poison (or 0)."""
    a = np.ascontiguousarray(images)
    if a.dtype not in (np.uint8, np.float32) or a.ndim not in (3, 4):
        raise ValueError("images must be u8 or f32 [n, h, w(, c)]")
    n, h = a.shape[:2]
    we = row_elems(a)
    if stride < we:
        raise ValueError(f"stride {stride} is shorter than a row of {we}")
    buf = np.zeros((n, h, stride), a.dtype)
    buf[:, :, :we] = a.reshape(n, h, we)
    if poisoned and stride > we:
        buf[:, :, we:] = poison(a.dtype, h, stride - we, we)[None]
    return buf.reshape(-1)


def compact(buf: np.ndarray, shape, stride: int) -> np.ndarray:
    """The dense images of a padded buffer; shape = the dense array's shape."""
    n, h = shape[:2]
    we = int(np.prod(shape[2:]))
    return np.ascontiguousarray(buf.reshape(n, h, stride)[:, :, :we]).reshape(shape)


def misread_pitch(buf: np.ndarray, shape, stride: int, image: int = 0) -> np.ndarray:
    """Image `image` as a reader sees it that steps rows by the dense row length instead of
    `stride` (from the image's right base, so it stays inside the buffer)."""
    h = shape[1]
    we = int(np.prod(shape[2:]))
    base = image * stride * h
    return buf[base:base + h * we].reshape((h,) + tuple(shape[2:])).copy()


def misread_clamp(buf: np.ndarray, shape, stride: int, image: int = 0, margin: int = 16):
    """Gray image `image` as a filter sees it that clamps columns to stride - 1 instead of the
    last used column (w & ~3) - 1: [h, (w & ~3) + margin], column c = the row's element
    min(c, stride - 1).  The margin is wider than the first level's filter radius."""
    n, h, w = shape
    tw = w & ~3
    rows = buf.reshape(n, h, stride)[image]
    cols = np.minimum(np.arange(tw + margin), stride - 1)
    return np.ascontiguousarray(rows[:, cols])
