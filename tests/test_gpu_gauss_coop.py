"""The paired Gaussian's cooperative strips (k_gauss_duo with COOP, DESIGN.md 4.10: the four waves
of a workgroup tile one 512-column window of level k+1 in LDS and read each other's halo columns,
one workgroup barrier per step) forced on every level where the form is compiled
(sgpu_debug_set_duo_strips, STRIPS_COOP), against one level per launch (SGPU_DEBUG_DUO_OFF): every
level of every octave and every keypoint, bit for bit -- no pixel's fma chain changes, only which
wave computes which column."""
import numpy as np
import pytest

import oracle_py as O
import sgpu
from sgpu_types import default_options
from sift_synth import synth_batch, synth_image

pytestmark = pytest.mark.gpu

DUO = sgpu.SiftContext.DEBUG_DUO_ALWAYS
DUO_OFF = sgpu.SiftContext.DEBUG_DUO_OFF
COOP = sgpu.SiftContext.STRIPS_COOP

# (n, w, h), the smallest shapes that reach each way the shared row can go wrong:
SHAPES = [
    (2, 16, 16),     # both edges in wave 0; waves 1-3 outside the image, still at the barriers
    (2, 116, 33),    # the right edge's clamped columns straddle the wave 0 / 1 boundary for
    (2, 120, 33),    # MOFF 12, 8 and 6 (116 + 12 = 120 + 8 = 128, 124 + 6 = 130); odd and
    (2, 124, 34),    # even heights
    (2, 480, 40),    # exact fits: one strip, two strips
    (1, 960, 41),
    (2, 500, 37),    # a last strip with only part of wave 0 inside the image
    (1, 964, 36),
    (3, 203, 97),    # ragged width
    (1, 1920, 72),   # the workload's width, kept short
]

_REF = {}   # (n, w, h) -> (images, levels of the first and last image, keypoints): one level per launch


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _levels(ctx, image, opts):
    geo = ctx.geometry()
    return [[ctx.gaussian(image, o, lvl).copy() for lvl in range(opts.dog_level_num + 3)]
            for o in range(len(geo))]


def _reference(ctx, n, w, h, opts):
    key = (n, w, h)
    if key not in _REF:
        imgs = synth_batch(n, w, h, 210 + w % 11)
        ctx.set_duo_strips(ctx.STRIPS_RULE)
        ctx.set_schedule()
        ctx.set_debug_flags(DUO_OFF)
        ctx.extract(imgs)
        ref = [_levels(ctx, i, opts) for i in (0, n - 1)]
        keys = [ctx.features(i)[0].copy() for i in range(n)]
        for lv in ref:
            for octave in lv:
                for a in octave:
                    a.setflags(write=False)
        _REF[key] = (imgs, ref, keys)
    return _REF[key]


# both pair plans: from the octave's end the u8 ingest pair (13, 11), (13, 17) with the second
# level decimated and (21, 25); from its front (11, 13) (and (17, 21), per-wave: not compiled in
# the cooperative form); band heights: auto, one chunk, not a multiple of 8
@pytest.mark.parametrize("pairs", [sgpu.SiftContext.PAIRS_END, sgpu.SiftContext.PAIRS_FRONT])
@pytest.mark.parametrize("rows", [0, 8, 36])
@pytest.mark.parametrize("n,w,h", SHAPES)
def test_coop_levels_equal_single_level(gpu_ctx, pairs, rows, n, w, h):
    opts = default_options()
    gpu_ctx.set_options(opts)
    try:
        imgs, ref, k_ref = _reference(gpu_ctx, n, w, h, opts)
        gpu_ctx.set_duo_strips(COOP)
        gpu_ctx.set_schedule(gpu_ctx.TRIO_OFF, pairs)
        gpu_ctx.set_debug_flags((rows << sgpu.SiftContext.DEBUG_BAND_SHIFT) | DUO)
        gpu_ctx.extract(imgs)
        got = [_levels(gpu_ctx, i, opts) for i in (0, n - 1)]
        for a, b in zip(ref, got):
            for o, (la, lb) in enumerate(zip(a, b)):
                for lvl, (x, y) in enumerate(zip(la, lb)):
                    assert np.array_equal(_bits(x), _bits(y)), (o, lvl)
        for i in range(n):
            assert np.array_equal(_bits(gpu_ctx.features(i)[0]), _bits(k_ref[i]))
    finally:
        gpu_ctx.set_duo_strips(gpu_ctx.STRIPS_RULE)
        gpu_ctx.set_schedule()
        gpu_ctx.set_debug_flags(0)


def test_coop_levels_vs_oracle(gpu_ctx):
    """The cooperative form's levels against the oracle (FilterH / FilterV, ProgramCU.cu:115-222),
    every level of every octave."""
    img = synth_image(640, 480, 1000)
    opts = default_options()
    gpu_ctx.set_options(opts)
    gpu_ctx.set_duo_strips(COOP)
    gpu_ctx.set_debug_flags(DUO)
    try:
        gpu_ctx.extract(img)
        for o in range(len(gpu_ctx.geometry())):
            for lvl in range(opts.dog_level_num + 3):
                g = gpu_ctx.gaussian(0, o, lvl)
                r = O.gaussian(img, o, lvl, opts)
                assert np.array_equal(_bits(g), _bits(r)), (o, lvl)
    finally:
        gpu_ctx.set_duo_strips(gpu_ctx.STRIPS_RULE)
        gpu_ctx.set_debug_flags(0)


def test_set_duo_strips_rejects_unknown_mode(gpu_ctx):
    with pytest.raises(Exception):
        gpu_ctx.set_duo_strips(3)
    gpu_ctx.set_duo_strips(gpu_ctx.STRIPS_RULE)
