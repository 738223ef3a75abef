"""The octaves' last Gaussian level, dense against lazy.

A lazy pyramid does not filter level nlev-1.  The wave-streaming extremum kernel decides DoG levels
0 .. d-2 from the planes it has, marks the undecided pixels of DoG level d-1 in the keypoint mask,
and k_extrema_top evaluates the level at their 3 x 3 neighbourhoods with the dense filter's
arithmetic, stores those values and runs the exact ComputeKEY test.  Everything after detection
must be the dense path's bit for bit: every case here runs one context with
SGPU_DEBUG_EXTREMA_TILE_OFF (the wave kernel at any size) in TOP_LEVEL_DENSE and in TOP_LEVEL_LAZY
and compares feature counts, keys, descriptors and candidates().  (A NaN on both sides counts as
equal.)  The test hooks are checked too: gaussian() of the last level after a lazy extract against
the oracle (the on-demand fill), the plan and the filter count, the rule mode on a cache-resident
batch, and the sparse evaluation alone (top_level_at) against the dense level's values.
"""
import numpy as np
import pytest

import oracle_py as O
import sgpu
import structured_images as SI
from sgpu_types import default_options
from sift_synth import synth_batch, synth_image

pytestmark = pytest.mark.gpu

C = sgpu.SiftContext
WAVE = C.DEBUG_EXTREMA_TILE_OFF


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    c = C(0, default_options())
    yield c
    c.close()


def _run(ctx, imgs, mode, opts, flags=WAVE):
    """counts, features, candidates, (launches, filters) and plan of one extract."""
    ctx.set_options(opts)
    ctx.set_top_level(mode)
    ctx.set_debug_flags(flags)
    try:
        ctx.extract(imgs)
        n = 1 if imgs.ndim == 2 else len(imgs)
        feats = [ctx.features(i) for i in range(n)]
        return ([ctx.count(i) for i in range(n)], feats, ctx.candidates(), ctx.pyramid_launches(),
                ctx.pyramid_plan())
    finally:
        ctx.set_debug_flags(0)
        ctx.set_top_level(C.TOP_LEVEL_RULE)


def _compare(ctx, imgs, opts=None, flags=WAVE, what=""):
    """Dense against lazy on one context; returns the two runs."""
    opts = opts or default_options()
    dense = _run(ctx, imgs, C.TOP_LEVEL_DENSE, opts, flags)
    lazy = _run(ctx, imgs, C.TOP_LEVEL_LAZY, opts, flags)
    assert dense[0] == lazy[0], f"{what}: feature counts"
    for i, ((dk, dd), (lk, ld)) in enumerate(zip(dense[1], lazy[1])):
        assert _same_bits(dk, lk), f"{what}: keys of image {i}"
        assert _same_bits(dd, ld), f"{what}: descriptors of image {i}"
    assert np.array_equal(dense[2][0], lazy[2][0]), f"{what}: candidate positions"
    assert _same_bits(dense[2][1][:, :3], lazy[2][1][:, :3]), f"{what}: candidate offsets"
    # the lazy run really left the level out: no plan entry writes it, one filter less per octave
    nlev, noct = opts.dog_level_num + 3, len(ctx.geometry())
    assert all(k != nlev - 1 for _, lv in lazy[4] for _, k in lv), what
    assert any(k == nlev - 1 for _, lv in dense[4] for _, k in lv), what
    assert lazy[3][1] == dense[3][1] - noct, what
    return dense, lazy


SHAPES = [(2, 16, 16, {}),            # smaller than the filter radius: every tap clamps on both sides
          (3, 203, 97, {}),           # rows 203 bytes apart: odd padding, one column per lane
          (1, 104, 33, {}),
          (2, 640, 480, dict(octave_num=4))]


@pytest.mark.parametrize("n,w,h,over", SHAPES, ids=lambda v: str(v))
def test_shapes(ctx, n, w, h, over):
    imgs = synth_batch(n, w, h, 50 + w % 11)
    dense, _ = _compare(ctx, imgs, default_options(**over), what=f"{n}x{w}x{h}")
    if w >= 100:
        assert sum(dense[0]) > 0


@pytest.mark.parametrize("over", [dict(dog_level_num=1), dict(dog_level_num=2),
                                  dict(dog_level_num=5), dict(filter_width_factor=5.5)],
                         ids=lambda v: str(v))
def test_options(ctx, over):
    """-d 1 (the only DoG level is the top one), 2, 5; -f 5.5 (filter widths up to 33)."""
    imgs = synth_batch(2, 203, 97, 61)
    dense, _ = _compare(ctx, imgs, default_options(**over), what=str(over))
    assert sum(dense[0]) > 0


@pytest.mark.parametrize("size", SI.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_structured_images(ctx, size):
    """Exact ties, saturation, few keys, float input that is large, negative, denormal or holds an
    Inf or a NaN pixel (tests/structured_images.py)."""
    for name in SI.ALL_IMAGES:
        _compare(ctx, SI.image(name, *size), what=name)


def test_nan_and_inf_pixels(ctx):
    """One NaN and one Inf pixel in a float image: a NaN DoG value is a candidate in the reference."""
    img = synth_image(203, 97, 7).astype(np.float32) / 255.0
    img[40, 100] = np.nan
    img[70, 30] = np.inf
    _compare(ctx, img, what="nan + inf")


def test_feature_count_limit(ctx):
    imgs = synth_batch(2, 320, 240, 71)
    full, _ = _compare(ctx, imgs, what="no limit")
    limit = max(8, min(full[0]) // 3)
    cut, _ = _compare(ctx, imgs, default_options(feature_count_threshold=limit), what="-tc")
    assert all(0 < c < f for c, f in zip(cut[0], full[0]))


def test_two_parts(ctx):
    _compare(ctx, synth_batch(3, 203, 97, 81), flags=WAVE | C.DEBUG_PARTS2, what="parts2")


def test_extract_stream(ctx):
    batches = [synth_batch(3, 203, 97, 90 + k) for k in range(2)]
    out = {}
    for mode in (C.TOP_LEVEL_DENSE, C.TOP_LEVEL_LAZY):
        ctx.set_options(default_options())
        ctx.set_top_level(mode)
        ctx.set_debug_flags(WAVE)
        try:
            out[mode] = ctx.extract_stream(batches, cap=20000)
        finally:
            ctx.set_debug_flags(0)
            ctx.set_top_level(C.TOP_LEVEL_RULE)
    (dk, dd, dc), (lk, ld, lc) = out[C.TOP_LEVEL_DENSE], out[C.TOP_LEVEL_LAZY]
    assert np.array_equal(dc, lc) and dc.sum() > 0
    assert _same_bits(dk, lk) and _same_bits(dd, ld)


@pytest.mark.parametrize("n,w,h,over", [(3, 203, 97, {}), (2, 640, 480, dict(octave_num=4))],
                         ids=lambda v: str(v))
def test_last_level_filled_on_demand(ctx, n, w, h, over):
    """After a lazy extract gaussian() still returns the whole last level of every octave."""
    imgs = synth_batch(n, w, h, 50 + w % 11)
    opts = default_options(**over)
    ctx.set_options(opts)
    ctx.set_top_level(C.TOP_LEVEL_LAZY)
    ctx.set_debug_flags(WAVE)
    try:
        ctx.extract(imgs)
        top = opts.dog_level_num + 2
        assert all(k != top for _, lv in ctx.pyramid_plan() for _, k in lv)
        keys = ctx.features(n - 1)[0].copy()
        for o in range(len(ctx.geometry())):
            for i in (0, n - 1):
                assert np.array_equal(_bits(ctx.gaussian(i, o, top)),
                                      _bits(O.gaussian(imgs[i], o, top, opts))), (o, i)
        # (a second request copies the level it already filled; the features are untouched)
        assert np.array_equal(_bits(ctx.gaussian(0, 0, top)), _bits(O.gaussian(imgs[0], 0, top, opts)))
        assert np.array_equal(_bits(ctx.features(n - 1)[0]), _bits(keys))
    finally:
        ctx.set_debug_flags(0)
        ctx.set_top_level(C.TOP_LEVEL_RULE)


def test_rule_is_dense_on_a_cache_resident_batch(ctx):
    """TOP_LEVEL_RULE goes lazy only where the size rule chooses the wave extremum kernel: a small
    batch keeps the dense plan, with the tile extremum kernel and with the wave kernel forced."""
    imgs = synth_batch(2, 203, 97, 61)
    opts = default_options()
    dense = _run(ctx, imgs, C.TOP_LEVEL_DENSE, opts, 0)
    for flags in (0, WAVE):
        rule = _run(ctx, imgs, C.TOP_LEVEL_RULE, opts, flags)
        assert rule[4] == dense[4] and rule[3] == dense[3]
    # TOP_LEVEL_LAZY with the tile extremum kernel is dense too
    lazy = _run(ctx, imgs, C.TOP_LEVEL_LAZY, opts, 0)
    assert lazy[4] == dense[4] and lazy[3] == dense[3]


@pytest.mark.parametrize("w,h", [(16, 16), (203, 97), (640, 480)])
def test_sparse_evaluation_equals_dense_level(ctx, w, h):
    """top_level_at (k_extrema_top's evaluation, alone) against the dense level's nine values: the
    interior's corners, a point within the filter radius of two borders, a mid-image point."""
    img = synth_image(w, h, 5)
    opts = default_options()
    ctx.set_options(opts)
    ctx.set_top_level(C.TOP_LEVEL_DENSE)
    try:
        ctx.extract(img)
        top = opts.dog_level_num + 2
        for o, (_, oh, wa) in enumerate(ctx.geometry()):
            g = ctx.gaussian(0, o, top).reshape(oh, wa)
            pts = {(1, 1), (wa - 2, oh - 2), (min(3, wa - 2), max(1, oh - 4)), (wa // 2, oh // 2)}
            for x, y in pts:
                got = ctx.top_level_at(0, o, x, y)
                assert np.array_equal(_bits(got), _bits(g[y - 1:y + 2, x - 1:x + 2])), (o, x, y)
    finally:
        ctx.set_top_level(C.TOP_LEVEL_RULE)
