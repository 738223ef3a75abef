"""What the structured images (tests/structured_images.py) contain, on the CPU oracle alone.

The GPU tests on these images (tests/test_gpu_structured.py) are worth what the images reach:
exact ties of neighbouring DoG values and of orientation peaks, full candidate rows, one keypoint,
clamped windows, non-finite float input.  The counts below are the oracle's at 320 x 240 and
203 x 97 with default options; a generator that changes silently changes them.

The tie rules themselves are shown to be reached by flipping one comparison of the oracle at a
time (ORACLE_TIE_VARIANT in oracle/sift_oracle.cpp, built on demand as oracle/liboracle_tie<N>.so):
each of T1, T2, T4 and T6 changes the features of a structured image, and none changes any of the
13 noise images the rest of the suite extracts from.
"""
import glob
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_py as O
import structured_images as SI
from sgpu_types import default_options
from sift_synth import synth_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")

# name -> (candidates, features) of the oracle, default options
COUNTS_320 = {
    "flat": (0, 0), "single": (1, 2), "disks_r2_p8": (1131, 2262), "blobs_half": (2, 4),
    "checker8": (697, 1394), "checker5_lowc": (216, 432), "binary_blocks4": (795, 1069),
    "binary_disks": (100, 170), "binary_disks_tied": (99, 162), "saturated_sines": (200, 393), "blobs_int": (5, 10),
    "ellipses_half": (3, 6), "border_ring": (12, 24),
    "f32_x1000": (1, 2), "f32_negated": (1, 2), "f32_denormal": (0, 0), "f32_inf": (22543, 2),
    "f32_nan": (35153, 2438),
}
COUNTS_203 = {
    "flat": (0, 0), "single": (1, 2), "disks_r2_p8": (264, 528), "blobs_half": (2, 4),
    "checker8": (186, 370), "checker5_lowc": (74, 148), "binary_blocks4": (188, 254),
    "binary_disks": (76, 101), "binary_disks_tied": (82, 122), "saturated_sines": (47, 89), "blobs_int": (7, 14),
    "ellipses_half": (3, 6), "border_ring": (10, 20),
    "f32_x1000": (2, 4), "f32_negated": (2, 4), "f32_denormal": (0, 0), "f32_inf": (13394, 2),
    "f32_nan": (20314, 2524),
}


def _extract(img, opts=None):
    return (O.extract_f32 if img.dtype == np.float32 else O.extract)(img, opts)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _locations(keys):
    """Distinct (x, y, scale) among the keys [n, 4]."""
    return {tuple(r) for r in keys[:, :3].view(np.uint32).tolist()}


@pytest.fixture(scope="module")
def results():
    """name -> (candidate ints, candidate floats, keys, descriptors) at 320 x 240 (not modified)."""
    def one(name):
        img = SI.image(name)
        return (name,) + O.candidates(img) + _extract(img)
    with ThreadPoolExecutor(8) as ex:
        return {r[0]: r[1:] for r in ex.map(one, SI.ALL_IMAGES)}


@pytest.mark.parametrize("name", list(SI.ALL_IMAGES))
def test_counts_320x240(results, name):
    ci, _, k, _ = results[name]
    assert (len(ci), len(k)) == COUNTS_320[name]


@pytest.mark.parametrize("name", list(SI.ALL_IMAGES))
def test_counts_203x97(name):
    img = SI.image(name, 203, 97)
    assert img.shape == (97, 203)
    assert (len(O.candidates(img)[0]), len(_extract(img)[0])) == COUNTS_203[name]


def test_generators_follow_their_formulas():
    """Spot values of the formulas, so that a reader can trust the names."""
    c = SI.checker8()
    assert c.dtype == np.uint8 and c[0, 0] == 0 and c[0, 8] == 255 and c[8, 8] == 0
    lc = SI.checker5_lowc()
    assert set(np.unique(lc)) == {100, 160} and lc[0, 5] == 160
    d = SI.disks_r2_p8()
    assert d[4, 4] == 255 and d[4, 6] == 255 and d[5, 6] == 0 and d[8, 8] == 0
    assert d.sum() == 255 * 13 * 30 * 40   # 13 pixels within radius 2 of each centre
    for name in ("binary_blocks4", "binary_disks"):
        assert set(np.unique(SI.image(name))) == {0, 255}
    s = SI.saturated_sines()
    assert (s == 0).mean() > 0.25 and (s == 255).mean() > 0.25   # plateaus at both ends
    assert SI.blobs_int()[120, 160] == 228 and SI.blobs_int()[120, 3] == 228
    h = SI.blobs_half()
    assert len(set(h[119:121, 159:161].ravel().tolist())) == 1   # the centre's 2 x 2 pixels tie
    assert np.all(SI.flat() == 128)
    for name in SI.U8_IMAGES:
        for w, hh in SI.SIZES:
            a = SI.image(name, w, hh)
            assert a.dtype == np.uint8 and a.shape == (hh, w), name
    nan, inf = SI.f32_nan(), SI.f32_inf()
    assert np.isnan(nan).sum() == 1 and np.isnan(nan[100, 100]) and np.isposinf(inf[100, 100])
    den = SI.f32_denormal()
    assert den.dtype == np.float32 and 0 < den.max() < 1e-29
    taps_product = den.max() * np.float32(1e-9)   # a far filter tap times a pixel
    assert 0 < taps_product < np.finfo(np.float32).tiny


def test_checker8_every_location_has_two_orientations(results):
    _, _, k, _ = results["checker8"]
    assert len(_locations(k)) == 697
    assert np.array_equal(_bits(k[0::2, :3]), _bits(k[1::2, :3]))
    assert not np.any(_bits(k[0::2, 3]) == _bits(k[1::2, 3]))


def test_checker5_lowc_fills_a_row(results):
    """A candidate at every fifth column: at least 60 in one row of one level (measured 62)."""
    ci = results["checker5_lowc"][0]
    rows, per_row = np.unique(ci[:, 1:3], axis=0, return_counts=True)
    assert per_row.max() >= 60
    row, lvl = rows[np.argmax(per_row)]
    cols = np.sort(ci[(ci[:, 1] == row) & (ci[:, 2] == lvl), 0])
    assert np.all(np.diff(cols) == 5)


def test_binary_blocks4_spans_levels(results):
    assert len(set(results["binary_blocks4"][0][:, 2].tolist())) >= 7


def test_single_has_one_location_in_the_last_rows(results):
    ci, _, k, _ = results["single"]
    assert len(k) == 2 and len(_locations(k)) == 1
    assert 240 - 10 < k[0, 1] < 240


def test_blob_near_a_border():
    """A 2.6-sigma blob 2 to 10 px from the left border gives two features at one location
    (3.04, 120.5 at 2 px); 1 px from it, or on it, none."""
    for d in range(0, 11):
        k, _ = O.extract(SI.border_blob(d))
        if d < 2:
            assert len(k) == 0, d
            continue
        assert len(k) == 2 and len(_locations(k)) == 1, d
        assert abs(k[0, 1] - 120.5) < 1e-3 and d < k[0, 0] < d + 1.1, (d, k[0])
    k, _ = O.extract(SI.border_blob(2))
    assert abs(k[0, 0] - 3.04) < 0.005


def test_border_ring_keys_at_every_distance(results):
    """Two features per blob; the nearest sit about 3 px from each of the four borders."""
    k = results["border_ring"][2]
    assert len(_locations(k)) == 12
    assert k[:, 0].min() < 3.1 and k[:, 1].min() < 3.1
    assert k[:, 0].max() > 320 - 3.1 and k[:, 1].max() > 240 - 3.1


def test_nan_pixel_gives_no_nan_features(results):
    ci, _, k, d = results["f32_nan"]
    assert len(k) > 2000
    assert not np.isnan(k).any() and not np.isnan(d).any()
    ki, di = results["f32_inf"][2:]
    assert len(ki) == 2 and not np.isnan(ki).any() and not np.isnan(di).any()


# ---- the tie rules -------------------------------------------------------------------------

TIE_VARIANTS = (1, 2, 3, 4, 6)
OPTION_SETS = ({}, {"max_orientation": 1})


def _suite_images():
    """The 13 noise images the other extraction tests use: the golden fixtures' and synth_image
    at the sizes and seeds of tests/test_gpu_parity.py."""
    gold = [np.load(p)["image"] for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden",
                                                                       "extract_*.npz")))]
    assert len(gold) == 7
    return gold + [synth_image(w, h, s) for w, h, s in
                   [(400, 300, 31), (640, 480, 1000), (333, 251, 9), (320, 240, 6), (203, 97, 2),
                    (160, 120, 1)]]


def _tie_images():
    return {(n, w, h): SI.image(n, w, h) for n in SI.U8_IMAGES for w, h in SI.SIZES}


def _keys_of(lib_path, images):
    """[[keys under each of OPTION_SETS] per image] from the oracle build at lib_path.  Keys
    only (descriptors off): every rule decides a key's presence or its orientation."""
    O.use_library(lib_path)
    try:
        O.lib()
        def one(img):
            return [O.extract(img, default_options(descriptors=0, **over))[0]
                    for over in OPTION_SETS]
        with ThreadPoolExecutor(8) as ex:
            return list(ex.map(one, images))
    finally:
        O.use_library(os.path.join(ORACLE_DIR, "liboracle.so"))


def _changed(a, b):
    """Per image: whether any option set's keys differ in count or bits."""
    return [any(x.shape != y.shape or not np.array_equal(_bits(x), _bits(y))
                for x, y in zip(p, q)) for p, q in zip(a, b)]


@pytest.fixture(scope="module")
def tie_runs():
    """variant -> (changed flags of the structured images, of the suite images); 0 -> names."""
    subprocess.check_call(["make", "-C", ORACLE_DIR, "liboracle.so"] +
                          [f"liboracle_tie{v}.so" for v in TIE_VARIANTS])
    structured, suite = _tie_images(), _suite_images()
    images = list(structured.values()) + suite
    base = _keys_of(os.path.join(ORACLE_DIR, "liboracle.so"), images)
    runs = {0: list(structured)}
    for v in TIE_VARIANTS:
        ch = _changed(base, _keys_of(os.path.join(ORACLE_DIR, f"liboracle_tie{v}.so"), images))
        runs[v] = (ch[:len(structured)], ch[len(structured):])
    return runs


@pytest.mark.parametrize("variant", [1, 2, 4, 6])
def test_tie_rule_is_reached(tie_runs, variant):
    """Flipping the rule changes the keys of a structured image, and of no suite image."""
    structured, suite = tie_runs[variant]
    caught = [n for n, c in zip(tie_runs[0], structured) if c]
    print(f"T{variant}: changes {caught}")
    assert ("checker8", 320, 240) in caught
    assert not any(suite), [i for i, c in enumerate(suite) if c]


def test_tie_rule_t3_is_not_reached(tie_runs):
    """T3 (a peak that equals the bin before it): no image here reaches it.  Two adjacent equal
    bins at a peak need a histogram that is mirror symmetric about a bin edge to the bit, and
    neither the accumulation in scan order nor the six (pre + v[j]) + v[j + 1] smoothing passes
    keep a mirror symmetry of the image exact (272 mirror-symmetric rectangles and ellipses at
    integer and half-integer centres, with and without subpixel refinement and the upsampled
    first octave, were tried as well: none).  Kept so that an image that does reach it (then
    add it to the structured images and assert as above) is noticed."""
    structured, suite = tie_runs[3]
    assert not any(structured) and not any(suite)
