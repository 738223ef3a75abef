"""Structured test images: exact ties, saturation, few keys, odd float input.

Every other extraction test draws its pixels from sift_synth.synth_image, whose Gaussian noise
keeps two neighbouring DoG values or two orientation bins from ever being bit-equal.  The images
here are noise free: symmetric patterns (equal DoG neighbours, equal histogram peaks), plateaus at
0 and 255 (gradients exactly zero inside a window), a candidate at every fifth column, one
keypoint location, blobs a few pixels from the border, and float input that is not a picture
scaled to [0, 1].  tests/test_structured_images.py holds what each image must contain (on the
oracle alone); tests/test_gpu_structured.py compares the HIP path with the oracle on them.

Pure functions of (w, h), u8 unless named f32_*; 320 x 240 is the size the formulas were written
for, other sizes scale the blob centres.
"""
import numpy as np


def _grid(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return yy, xx


def _blob(w, h, cx, cy, s, a=100.0):
    yy, xx = _grid(w, h)
    return a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * s * s))


def _ellipse(w, h, cx, cy, sx, sy, a):
    yy, xx = _grid(w, h)
    return a * np.exp(-((xx - cx) ** 2 / (2.0 * sx * sx) + (yy - cy) ** 2 / (2.0 * sy * sy)))


def _u8(a):
    return np.rint(np.clip(a, 0, 255)).astype(np.uint8)


def _sx(w, x):
    """Column x of the 320-wide formula at width w, an integer."""
    return int(np.floor(x * w / 320.0 + 0.5))


def _sy(h, y):
    return int(np.floor(y * h / 240.0 + 0.5))


def checker8(w=320, h=240):
    yy, xx = _grid(w, h)
    return (((xx // 8 + yy // 8) % 2) * 255).astype(np.uint8)


def checker5_lowc(w=320, h=240):
    yy, xx = _grid(w, h)
    return (100 + ((xx // 5 + yy // 5) % 2) * 60).astype(np.uint8)


def disks_r2_p8(w=320, h=240):
    yy, xx = _grid(w, h)
    img = np.zeros((h, w), np.uint8)
    for cy in range(4, h, 8):
        for cx in range(4, w, 8):
            img[(yy - cy) ** 2 + (xx - cx) ** 2 <= 4] = 255
    return img


def binary_blocks4(w=320, h=240):
    """Random 4 x 4 blocks of 0 / 255 (columns and rows past the last whole block are 0)."""
    cells = np.random.default_rng(1).integers(0, 2, (h // 4, w // 4)) * 255
    img = np.zeros((h, w), np.uint8)
    img[:h // 4 * 4, :w // 4 * 4] = np.kron(cells, np.ones((4, 4), np.int64))
    return img


def _disks(w, h, rng):
    yy, xx = _grid(w, h)
    img = np.zeros((h, w), np.uint8)
    for i in range(150):
        cx = rng.uniform(0, w)
        cy = rng.uniform(0, h)
        r = rng.uniform(2, 9)
        img[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 255 * (i % 2)
    return img


def binary_disks(w=320, h=240):
    """150 disks, alternately 0 and 255, later ones over earlier ones, on 0.  The generator is
    binary_blocks4's after its draw: at 320 x 240 that stream gives an image without exact ties
    (the float64 restatement finds the oracle's 100 candidates, tests/test_ref_numpy.py)."""
    rng = np.random.default_rng(1)
    rng.integers(0, 2, (h // 4, w // 4))
    return _disks(w, h, rng)


def binary_disks_tied(w=320, h=240):
    """The same from a fresh default_rng(1).  At 320 x 240 four of its small disks lie mirror
    symmetric about a pixel boundary, and the two equal DoG values at each centre are told apart
    by the comparison order alone (4 of the oracle's 99 candidates are the float64
    restatement's neighbour instead)."""
    return _disks(w, h, np.random.default_rng(1))


def saturated_sines(w=320, h=240):
    yy, xx = _grid(w, h)
    return _u8(128 + 400 * np.sin(xx / 7 + 0.3) * np.sin(yy / 5 + 0.1 * xx / 7))


def blobs_int(w=320, h=240):
    """Blobs at integer centres; the last two stay 3 px from the left and the bottom border."""
    return _u8(128 + _blob(w, h, _sx(w, 160), _sy(h, 120), 4) +
               _blob(w, h, _sx(w, 60), _sy(h, 60), 2.6) +
               _blob(w, h, _sx(w, 250), _sy(h, 180), 6) +
               _blob(w, h, 3, _sy(h, 120), 2.6) + _blob(w, h, _sx(w, 160), h - 4, 2.6))


def blobs_half(w=320, h=240):
    """Blobs centred between pixels: the 2 x 2 pixels around a centre are equal."""
    return _u8(128 + _blob(w, h, _sx(w, 160) - 0.5, _sy(h, 120) - 0.5, 4) +
               _blob(w, h, _sx(w, 60) + 0.5, _sy(h, 60) + 0.5, 2.6) +
               _blob(w, h, _sx(w, 250) + 0.5, _sy(h, 180), 6))


def ellipses_half(w=320, h=240):
    """Anisotropic Gaussians of amplitude +100, -100, +100 centred between pixels on one axis
    or on both."""
    return _u8(128 + _ellipse(w, h, _sx(w, 40), _sy(h, 40) + 0.5, 2.6, 5, 100.0) +
               _ellipse(w, h, _sx(w, 140) + 0.5, _sy(h, 120), 5, 2.6, -100.0) +
               _ellipse(w, h, _sx(w, 240) + 0.5, _sy(h, 190) + 0.5, 3, 4, 100.0))


BORDER_DISTANCES = (2, 3, 5)


def border_ring(w=320, h=240):
    """2.6-sigma blobs whose centres lie 2, 3 and 5 px from each of the four borders, 40 px
    apart around the border's middle: their orientation and descriptor windows clamp."""
    a = np.full((h, w), 128.0)
    for k, d in enumerate(BORDER_DISTANCES):
        x, y = w // 2 + 40 * (k - 1), h // 2 + 40 * (k - 1)
        a += _blob(w, h, d, y, 2.6) + _blob(w, h, w - 1 - d, y, 2.6)
        a += _blob(w, h, x, d, 2.6) + _blob(w, h, x, h - 1 - d, 2.6)
    return _u8(a)


def border_blob(d, w=320, h=240):
    """One 2.6-sigma blob d px from the left border, at half height."""
    return _u8(128 + _blob(w, h, d, h // 2, 2.6))


def single(w=320, h=240):
    """One keypoint location, in the last rows."""
    return _u8(128 + _blob(w, h, w - 19.7, h - 9.3, 2.6))


def flat(w=320, h=240):
    return np.full((h, w), 128, np.uint8)


def _f32_base(w, h):
    return ((128 + _blob(w, h, _sx(w, 160), _sy(h, 120), 4)) / 255).astype(np.float32)


def _f32_pixel(w, h):
    """(row, column) of the one non-finite pixel: (100, 100) at 320 x 240."""
    return _sy(h, 100), _sx(w, 100)


def f32_x1000(w=320, h=240):
    return _f32_base(w, h) * np.float32(1000)


def f32_negated(w=320, h=240):
    return -_f32_base(w, h)


def f32_denormal(w=320, h=240):
    """Pixels near 1e-30: the filter taps' products and the DoG values are denormal."""
    return _f32_base(w, h) * np.float32(1e-30)


def f32_inf(w=320, h=240):
    a = _f32_base(w, h)
    a[_f32_pixel(w, h)] = np.inf
    return a


def f32_nan(w=320, h=240):
    a = _f32_base(w, h)
    a[_f32_pixel(w, h)] = np.nan
    return a


# In the order of the batch test (tests/test_gpu_structured.py): empty, two features, thousands,
# a few, ...
U8_IMAGES = {f.__name__: f for f in (
    flat, single, disks_r2_p8, blobs_half, checker8, checker5_lowc, binary_blocks4, binary_disks,
    binary_disks_tied, saturated_sines, blobs_int, ellipses_half, border_ring)}
F32_IMAGES = {f.__name__: f for f in (f32_x1000, f32_negated, f32_denormal, f32_inf, f32_nan)}
# Images whose candidate set is decided by float32 rounding and the tie order (symmetric
# patterns); the others are tie free as far as the float64 restatement can tell.
TIE_IMAGES = ("checker8", "checker5_lowc", "disks_r2_p8", "binary_disks_tied", "blobs_int",
              "blobs_half", "ellipses_half")
ALL_IMAGES = {**U8_IMAGES, **F32_IMAGES}
SIZES = ((320, 240), (203, 97))


def image(name, w=320, h=240):
    return ALL_IMAGES[name](w, h)
