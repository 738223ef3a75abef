"""The HIP path against the CPU oracle on the structured images (tests/structured_images.py):
exact ties of DoG neighbours and of orientation peaks, plateaus at 0 and 255, full candidate rows,
one keypoint, windows clamped at the border, and float input that is large, negative, denormal or
holds one Inf or NaN pixel.  tests/test_structured_images.py shows on the oracle alone that the
images contain these, and that they reach the tie rules no noise image reaches.

On the images with ties, bitwise parity pins the documented tie rules (the READ_CMP_DOG_DATA
order, the strict > chains of the orientation peaks) as the oracle states them -- the float64
restatement agrees with the oracle on a tenth of checker8's candidates, so float32 rounding and
the comparison order decide the set.

Every form of the pipeline is compared with the oracle itself, not only with another form:
candidates (integers equal, offsets bitwise), keys bitwise, descriptors bitwise from the exact
kernel, and the shipped descriptor within L2 1e-5 of the exact kernel and DESC_L2_TOL of the
oracle with the exact run's keys.  NaN payloads are not compared.  Shapes: 320 x 240, and the
same formulas at 203 x 97 (ragged tiles, partial waves, a width that is no multiple of 4).
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_py as O
import sgpu
import structured_images as SI
from sgpu_types import default_options

pytestmark = pytest.mark.gpu

C = sgpu.SiftContext
DESC_L2_TOL = 1e-4    # BASELINE.json north_star (tests/test_gpu_parity.py)
FAST_L2_TOL = 1e-5    # shipped descriptor against the exact kernel (test_shipped_descriptor_vs_exact)
GRID = 12             # workgroups per kernel of the capped feature-queue context
CASES = [(n, w, h) for w, h in SI.SIZES for n in SI.ALL_IMAGES]


def _id(case):
    return f"{case[0]}-{case[1]}x{case[2]}"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    """Bit equality, a NaN on both sides counting as equal."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _l2(d, rd):
    """Largest row distance over the rows that are finite on the reference side, which must be
    the finite rows of d too."""
    if len(rd) == 0:
        return 0.0
    ok = np.isfinite(rd).all(1)
    assert np.array_equal(np.isfinite(d).all(1), ok)
    if not ok.any():
        return 0.0
    return float(np.linalg.norm(d[ok].astype(np.float64) - rd[ok].astype(np.float64), axis=1).max())


def _oracle(img, opts=None):
    """(candidate ints, candidate offsets, keys, descriptors) of the oracle."""
    ext = O.extract_f32 if img.dtype == np.float32 else O.extract
    return O.candidates(img, opts) + ext(img, opts)


@pytest.fixture(scope="module")
def refs():
    """(name, w, h) -> (image, oracle result), default options: computed once, not modified."""
    def one(case):
        img = SI.image(*case)
        return case, (img, _oracle(img))
    with ThreadPoolExecutor(8) as ex:
        return dict(ex.map(one, CASES))


@pytest.fixture(scope="module")
def ctxs(gpu_ctx):
    """(quad, queue): contexts created with SGPU_WAVE_ORIENT_MAX=0, which keep the quad
    orientation kernel for any candidate count; `queue` also with SGPU_FEATURE_QUEUE_GRID=12, so
    that all but the first 12 candidate groups and features are handed out by the work counters."""
    names = ("SGPU_WAVE_ORIENT_MAX", "SGPU_FEATURE_QUEUE_GRID")
    old = {k: os.environ.get(k) for k in names}
    os.environ["SGPU_WAVE_ORIENT_MAX"] = "0"
    os.environ.pop("SGPU_FEATURE_QUEUE_GRID", None)
    try:
        quad = C(0, default_options())
        os.environ["SGPU_FEATURE_QUEUE_GRID"] = str(GRID)
        queue = C(0, default_options())
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield quad, queue
    quad.close()
    queue.close()


def _extract(ctx, img, flags=0):
    """[(keys, descriptors)] per image of one extract under the debug flags."""
    ctx.set_debug_flags(flags)
    try:
        ctx.extract(img)
        return [ctx.features(i) for i in range(1 if img.ndim == 2 else len(img))]
    finally:
        ctx.set_debug_flags(0)


def _check_features(ctx, img, ref, flags=0, what=""):
    """One image through ctx under `flags`: the shipped and the exact descriptor run."""
    rk, rd = ref[2], ref[3]
    k, d = _extract(ctx, img, flags)[0]
    assert _same_bits(k, rk), f"{what}: keys differ from the oracle ({k.shape} / {rk.shape})"
    ke, de = _extract(ctx, img, flags | C.DEBUG_EXACT_DESCRIPTOR)[0]
    assert _same_bits(ke, rk), f"{what}: exact run's keys differ from the oracle"
    assert _same_bits(de, rd), f"{what}: exact descriptors differ from the oracle"
    assert _same_bits(k, ke), what
    assert _l2(d, rd) < DESC_L2_TOL, what
    assert _l2(d, de) < FAST_L2_TOL, what


# The images with an Inf or a NaN pixel: also test_shipped_descriptor_with_nonfinite_pixels.
NONFINITE = ("f32_inf", "f32_nan")


def _check_candidates(ctx, ref, what=""):
    gi, gf = ctx.candidates()
    assert np.array_equal(gi, ref[0]), what
    assert _same_bits(gf[:, :3], ref[1][:, :3]), what   # column 3 is padding


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_shipped_path(gpu_ctx, refs, case):
    """The shipped single-image path.  A call's grids and kernel forms come from the counts of
    the call before it (one wave per candidate up to 16384 candidates, a workgroup per feature
    for few features): the first extract here follows another image's, the later ones the
    image's own.  For float input also the levels, where a flush to zero or a max() that drops
    a NaN would show first."""
    img, ref = refs[case]
    gpu_ctx.set_options(default_options())
    gpu_ctx.set_debug_flags(0)
    gpu_ctx.extract(img)
    _check_candidates(gpu_ctx, ref, "after another image")
    _check_features(gpu_ctx, img, ref, 0, "shipped")
    gpu_ctx.extract(img)
    _check_candidates(gpu_ctx, ref, "steady state")
    if img.dtype == np.float32:
        for o, lvl in ((0, 0), (0, 1), (1, default_options().dog_level_num + 2)):
            assert _same_bits(gpu_ctx.gaussian(0, o, lvl), O.gaussian(img, o, lvl)), (o, lvl)


FORMS = {
    "extrema_tile_off": C.DEBUG_EXTREMA_TILE_OFF,
    "gauss_tile_always": C.DEBUG_GAUSS_TILE_ALWAYS,
    "gauss_tile_off": C.DEBUG_GAUSS_TILE_OFF,
    "duo_off": C.DEBUG_DUO_OFF,
    "orient_wave": C.DEBUG_ORIENT_WAVE,
    "desc_wide_always": C.DEBUG_DESC_WIDE_ALWAYS,
    "desc_wide_off": C.DEBUG_DESC_WIDE_OFF,
}


@pytest.mark.parametrize("size", SI.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("form", list(FORMS))
def test_forms(gpu_ctx, refs, form, size):
    """Every image under one forced kernel form, against the oracle."""
    gpu_ctx.set_options(default_options())
    for name in SI.ALL_IMAGES:
        img, ref = refs[(name,) + size]
        _check_features(gpu_ctx, img, ref, FORMS[form], f"{form} {name}")
        gpu_ctx.set_debug_flags(FORMS[form])
        gpu_ctx.extract(img)
        gpu_ctx.set_debug_flags(0)
        _check_candidates(gpu_ctx, ref, f"{form} {name}")


@pytest.mark.parametrize("size", SI.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_quad_orientation(ctxs, refs, size):
    """The quad orientation kernel (a context that never takes the one-wave form), with the
    one-wave descriptor kernel, on every image."""
    quad = ctxs[0]
    quad.set_options(default_options())
    quad.set_feature_queue(C.FEATURES_QUEUE)
    for name in SI.ALL_IMAGES:
        img, ref = refs[(name,) + size]
        _check_features(quad, img, ref, C.DEBUG_DESC_WIDE_OFF, f"quad {name}")


@pytest.mark.parametrize("size", SI.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_feature_queue(ctxs, refs, size):
    """The persistent feature stages with 12 workgroups per kernel against the oracle and against
    FEATURES_STATIC; each compared extract follows an extract of another image of the same shape
    on the same context (advanced counters, other bits in the rows)."""
    quad, queue = ctxs
    names = list(SI.ALL_IMAGES)
    for c in (quad, queue):
        c.set_options(default_options())
    quad.set_feature_queue(C.FEATURES_STATIC)
    queue.set_feature_queue(C.FEATURES_QUEUE)
    try:
        for i, name in enumerate(names):
            img, ref = refs[(name,) + size]
            other = refs[(names[i - 1],) + size][0]
            _extract(queue, other, C.DEBUG_DESC_WIDE_OFF)
            _check_features(queue, img, ref, C.DEBUG_DESC_WIDE_OFF, f"queue {name}")
            _extract(queue, other, C.DEBUG_DESC_WIDE_OFF)
            q = _extract(queue, img, C.DEBUG_DESC_WIDE_OFF)[0]
            s = _extract(quad, img, C.DEBUG_DESC_WIDE_OFF)[0]
            assert _same_bits(s[0], ref[2]), f"static {name}"
            assert _same_bits(q[0], s[0]) and _same_bits(q[1], s[1]), f"queue / static {name}"
    finally:
        quad.set_feature_queue(C.FEATURES_QUEUE)


@pytest.mark.parametrize("size", SI.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", NONFINITE)
def test_shipped_descriptor_with_nonfinite_pixels(gpu_ctx, ctxs, refs, name, size):
    """The shipped descriptor kernel (k_descriptor_flat and its queue / wide forms) on the images
    with one Inf or NaN pixel, under every form: the bounds of every other image (L2 1e-5 of the
    exact kernel, DESC_L2_TOL of the oracle).

    The reference adds a window sample's weight whatever its value (ProgramCU.cu:1054-1082), so
    one NaN sample makes the squared norm NaN, every component min(0.2, NaN) = 0.2 (CUDA's fminf
    drops the NaN, sift_math.h:30) and the descriptor uniform, 1 / sqrt(128) (:1173-1208); an
    Inf sample leaves 0.2 in its bins and 0 elsewhere.  The oracle and the exact kernel do the
    same, bit for bit.  The shipped kernels sum 32.32 fixed-point integers, which cannot carry
    that: they flag a window that holds a weight that is not finite and k_descriptor_nonfinite
    computes the flagged rows with the exact kernel's code.  Before that these rows differed by
    L2 up to 1.32 (f32_nan: 2436 of 2438 rows at 320 x 240, all 2524 at 203 x 97; f32_inf: both
    rows at 203 x 97, 0.316 in 10 bins against the uniform row) under every form.  Every figure
    is printed before it is asserted."""
    quad, queue = ctxs
    img, ref = refs[(name,) + size]
    runs = [("shipped", gpu_ctx, 0)] + [(f, gpu_ctx, v) for f, v in FORMS.items()]
    runs += [("quad", quad, C.DEBUG_DESC_WIDE_OFF), ("queue", queue, C.DEBUG_DESC_WIDE_OFF)]
    worst = []
    for what, ctx, flags in runs:
        ctx.set_options(default_options())
        ctx.set_feature_queue(C.FEATURES_QUEUE)
        _extract(ctx, img, flags)
        (k, d), = _extract(ctx, img, flags)
        (ke, de), = _extract(ctx, img, flags | C.DEBUG_EXACT_DESCRIPTOR)
        assert _same_bits(k, ref[2]) and _same_bits(de, ref[3]), what
        dist = np.linalg.norm(d.astype(np.float64) - ref[3].astype(np.float64), axis=1)
        dist_e = np.linalg.norm(d.astype(np.float64) - de.astype(np.float64), axis=1)
        print(f"{name} {size} {what}: {len(k)} features, shipped descriptor L2 to the oracle max "
              f"{np.nanmax(dist):.3g} ({int((~(dist < DESC_L2_TOL)).sum())} rows over), to the "
              f"exact kernel max {np.nanmax(dist_e):.3g} ({int((~(dist_e < FAST_L2_TOL)).sum())} "
              f"rows over), non-finite rows {int((~np.isfinite(d).all(1)).sum())}")
        worst.append((what, float(np.nanmax(dist)), float(np.nanmax(dist_e)),
                      bool(np.isfinite(d).all())))
    assert all(fin and a < DESC_L2_TOL and b < FAST_L2_TOL for _, a, b, fin in worst), worst


@pytest.mark.parametrize("flags", [0, C.DEBUG_PARTS2], ids=["shipped", "parts2"])
def test_batch_of_all_u8_images(gpu_ctx, refs, flags):
    """One batch of every u8 320 x 240 image -- an empty one, a two-feature one and a
    2262-feature one first -- under the shipped schedule and split into two parts."""
    names = list(SI.U8_IMAGES)
    assert names[:5] == ["flat", "single", "disks_r2_p8", "blobs_half", "checker8"]
    batch = np.stack([refs[(n, 320, 240)][0] for n in names])
    want = [refs[(n, 320, 240)][1] for n in names]
    assert [len(r[2]) for r in want][:5] == [0, 2, 2262, 4, 1394]
    gpu_ctx.set_options(default_options())
    got = _extract(gpu_ctx, batch, flags)
    assert [len(k) for k, _ in got] == [len(r[2]) for r in want]
    assert gpu_ctx.total() == sum(len(r[2]) for r in want)
    exact = _extract(gpu_ctx, batch, flags | C.DEBUG_EXACT_DESCRIPTOR)
    for name, (k, d), (ke, de), r in zip(names, got, exact, want):
        assert _same_bits(k, r[2]) and _same_bits(ke, r[2]), name
        assert _same_bits(de, r[3]), name
        assert _l2(d, r[3]) < DESC_L2_TOL and _l2(d, de) < FAST_L2_TOL, name


OPTION_CASES = [
    {"max_orientation": 1},
    {"subpixel": 0},
    {"keep_extremum_sign": 1},
    {"fixed_orientation": 1},
    {"circular_window": 1},
    {"dog_level_num": 5},
    {"octave_min": -1},   # the upsampled image of a symmetric pattern has more ties
    {"octave_min": 1},
]


@pytest.mark.parametrize("name", ["checker8", "blobs_half", "disks_r2_p8"])
@pytest.mark.parametrize("over", OPTION_CASES, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_options(gpu_ctx, refs, over, name):
    img = refs[(name, 320, 240)][0]
    opts = default_options(**over)
    ref = _oracle(img, opts)
    gpu_ctx.set_options(opts)
    try:
        gpu_ctx.extract(img)
        _check_candidates(gpu_ctx, ref, str(over))
        _check_features(gpu_ctx, img, ref, 0, f"{name} {over}")
    finally:
        gpu_ctx.set_options(default_options())
