"""The CPU oracle against the reference's own CUDA kernels, run on the host.

oracle/_ref/libref_kernels.so (built by oracle/Makefile where a checkout of the reference is
present) holds the reference's ProgramCU.cu, compiled for the CPU through oracle/cuda_host, and
tests/ref_kernels.py calls its stage functions one by one.  Every stage gets the *oracle's*
output of the stage before it, so a rounding difference cannot cascade into set differences.

Two halves: the live comparisons need the library and skip without it; the fixture comparisons
(tests/golden/ref_*.npz, recorded from the library by tests/make_ref_golden.py) always run, and
where the library is present the fixtures are also compared with a live run.

Exact stages (integers, or comparisons and subtractions of identical floats) are asserted equal.
Float stages pass when the oracle's distance from the library built with -ffp-contract=off is at
most 2 * max(A, C):
  A  the distance between the -ffp-contract=off and -ffp-contract=fast builds of the reference
     (nvcc's fma choices are unknown; the two builds bracket them),
  C  the distance between liboracle.so and liboracle_perturb.so on the same stage (CUDA's
     documented device-function errors, oracle/perturb.h),
both measured on the inputs of the test and recorded below with B, the oracle's measured
distance (run with -s to see all three again).  The factor 2 covers a libm that differs by an
ulp between machines.
"""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import oracle_py as O
import ref_cases as C
import ref_kernels as R
import structured_images as SI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
GOLDEN = os.path.join(ROOT, "tests", "golden")
live = pytest.mark.skipif(not R.available(),
                          reason="oracle/_ref/libref_kernels.so not built: build() found no "
                                 "reference checkout")

# name: (A ref off vs fast, B ref vs oracle, C oracle vs perturbed oracle), max abs unless said
MEASURED = {
    "filter": (2.38e-7, 2.38e-7, 0.0),
    "upsample": (0.0, 0.0, 0.0),
    "gradient_magnitude": (2.98e-8, 2.98e-8, 0.0),
    "gradient_angle": (0.0, 2.38e-7, 7.15e-7),              # radians
    "key_offset": (1.49e-7, 1.49e-7, 0.0),                  # pixels, levels
    "key_scale_rel": (0.0, 1.19e-7, 2.98e-7),
    "orientation_angle": (0.0, 0.0, 9.59e-5),               # radians (one step of the 16-bit packing)
    "descriptor_l2": (8.25e-7, 1.01e-6, 2.39e-6),           # window factors 3 and 2
    "descriptor_unnormalized_rel": (1.43e-6, 1.44e-6, 1.85e-6),   # L2 over the reference's norm
    "descriptor_rect_l2": (1.26e-6, 1.25e-6, 3.32e-7),
}
# tests/test_ref_numpy.py holds the same quantities to 2e-5 (levels), 1e-3 (offsets), 2e-3 rad
# and 1e-4 (descriptors): every bound here is tighter.


def tol(name):
    a, _, c = MEASURED[name]
    return 2.0 * max(a, c)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@contextlib.contextmanager
def oracle_library(name):
    """Bind another build of the oracle (liboracle_perturb.so, liboracle_tie<N>.so)."""
    path = os.path.join(ORACLE_DIR, name)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ORACLE_DIR, name])
    O.use_library(path)
    try:
        yield
    finally:
        O.use_library(os.path.join(ORACLE_DIR, "liboracle.so"))


def _perturbed(fn):
    with oracle_library("liboracle_perturb.so"):
        return fn()


def _report(name, a, b, c):
    """Print the three measured distances of a stage; A and C, which set the bound, must still be
    what MEASURED records (within the factor 2 that the bound itself allows a libm)."""
    print(f"{name}: A ref off/fast {a:.3g}  B ref/oracle {b:.3g}  C oracle/perturbed {c:.3g}  "
          f"bound {tol(name):.3g}")
    ra, _, rc = MEASURED[name]
    assert a <= 2.0 * ra and c <= 2.0 * rc, (name, a, ra, c, rc)


# =============================================================================================
# exact stages
# =============================================================================================

def _oracle_match(q1, q2, kw, mbm, max_match=None):
    return O.match(q1, q2, kw.get("distmax", 0.7), kw.get("ratiomax", 0.8), mbm, max_match)


@live
@pytest.mark.parametrize("name", C.MATCH_LIVE)
def test_matcher(name):
    """O.match = MultiplyDescriptor -> GetRowMatch -> GetColMatch, with and without the mutual
    check (the row decisions are the same kernel launch for both)."""
    q1, q2, kw = C.match_case(name)
    small = len(q1) * len(q2) <= 1 << 20   # the dot products themselves, where that is cheap
    row, col, dot = R.match_stages(q1, q2, mbm=1, want_dot=small, **kw)
    if small:
        assert np.array_equal(dot, q1.astype(np.int32) @ q2.astype(np.int32).T)
    for mbm in (0, 1):
        want = R.pairs(row, col if mbm else None)
        np.testing.assert_array_equal(_oracle_match(q1, q2, kw, mbm), want, err_msg=f"mbm {mbm}")
    if name == "tie_70x100":   # the tie winners show without the mutual check
        assert len(R.pairs(row, None)) >= 5


@live
def test_matcher_max_match():
    q1, q2, kw = C.match_case("size_257_1000_100")
    row, col, _ = R.match_stages(q1, q2, mbm=1)
    full = R.pairs(row, col)
    assert len(full) > 20
    for cap in (0, 1, 10, len(full), len(full) + 5):
        np.testing.assert_array_equal(O.match(q1, q2, max_match=cap), R.pairs(row, col, cap))


def _guided(name, lib_match):
    q1, q2, l1, l2, H, F, kw = C.guided_case(name)
    kw = {k: v for k, v in kw.items() if k != "planted"}
    return lib_match(q1, q2, l1, l2, H, F, kw)


def _ref_guided(q1, q2, l1, l2, H, F, kw, fast=False):
    return R.match(q1, q2, kw["distmax"], kw["ratiomax"], kw["mbm"], loc1=l1, loc2=l2, H=H, F=F,
                   hdistmax=kw["hdistmax"], fdistmax=kw["fdistmax"], fast=fast)


def _oracle_guided(q1, q2, l1, l2, H, F, kw):
    return O.match_guided(q1, q2, l1, l2, H, F, distmax=kw["distmax"], ratiomax=kw["ratiomax"],
                          hdistmax=kw["hdistmax"], fdistmax=kw["fdistmax"], mbm=kw["mbm"])


@live
@pytest.mark.parametrize("name", C.GUIDED_LIVE)
def test_guided_matcher(name):
    """O.match_guided = MultiplyDescriptorG and the same two kernels; set sizes 301, 173 and 9 are
    no multiples of the 8-row block.  The geometric test is float arithmetic: the scenes keep
    every pair away from its thresholds, which the two contraction builds agreeing shows."""
    want = _guided(name, _ref_guided)
    np.testing.assert_array_equal(_guided(name, lambda *a: _ref_guided(*a, fast=True)), want)
    np.testing.assert_array_equal(_guided(name, _oracle_guided), want)
    if name == "block_rule":
        assert list(C.guided_case(name)[6]["planted"]) in want.tolist()
    elif C.guided_case(name)[0].shape[0] > 100:
        assert len(want) > 10


@live
@pytest.mark.parametrize("name", sorted(C.FLOAT_IMAGES))
def test_dog_values(name):
    """One subtraction of identical inputs: bit for bit."""
    for (o, j), st in C.levels(name).items():
        h, wa = st["dog"].shape[1:]
        g = [O.gaussian(C.image(name), o, m).reshape(h, wa) for m in (j, j + 1)]
        d, _ = R.dog(g[0], g[1])
        assert np.array_equal(_bits(d), _bits(O.stage_dog(g[0], g[1])[0])), (o, j)
        assert np.array_equal(_bits(d), _bits(st["dog"][0])), (o, j)


@live
@pytest.mark.parametrize("w,h,count", C.LIST_CASES)
def test_histogram_pyramid_and_list(w, h, count):
    """InitHistogram / ReduceHistogram / GenerateList on a key image: the reference's list is
    the oracle's, in order, at histogram widths 127, 128, 129 and list lengths 127 ... 300."""
    key = C.key_image(w, h, count, 7 * w + h)
    widths = O.hist_widths(w, h)
    assert widths[0] == w // 4
    lst, hists = R.feature_list(key, widths)
    assert int(hists[-1].sum()) == count == len(lst)
    want = O.stage_list(key)
    np.testing.assert_array_equal(lst[:, :2], want[:, :2])
    assert not lst[:, 2:].any()


@live
@pytest.mark.parametrize("name", sorted(C.FLOAT_IMAGES) + list(SI.TIE_IMAGES))
def test_pipeline_list_is_the_reference_list(name):
    """The list the oracle's pipeline hands to orientation (and to everything after it), for
    every level of two octaves: the reference's three kernels on the pipeline's own key image give
    it, in order, and so does the oracle's stand-alone stage.  The second octave's histogram
    pyramid takes its depth from the first octave's size."""
    stages = C.levels(name)
    h0, w0 = stages[(0, 0)]["key"].shape[:2]
    total = 0
    for (o, j), st in stages.items():
        h, wa = st["key"].shape[:2]
        lst, _ = R.feature_list(st["key"], O.hist_widths(wa, h, (w0, h0)))
        np.testing.assert_array_equal(lst, st["list"], err_msg=f"{name} {o} {j}")
        np.testing.assert_array_equal(O.stage_list(st["key"], (w0, h0)), st["list"])
        total += len(lst)
    assert total > 0


def _key_signs(st, oracle=True, fast=False):
    d = st["dog"]
    if oracle:
        return O.stage_key(d[0], d[1], d[2], st["tdog"], st["tedge"])
    return R.key(d[0], d[1], d[2], st["tdog"], st["tedge"], fast=fast)


def _check_tie_keys(name):
    total = 0
    for (o, j), st in C.levels(name).items():
        ref = _key_signs(st, oracle=False)
        got = _key_signs(st)
        assert np.array_equal(ref[..., 0], got[..., 0]), (name, o, j)
        total += int(np.count_nonzero(ref[..., 0]))
    return total


@live
@pytest.mark.parametrize("name", SI.TIE_IMAGES)
def test_extremum_decisions_on_tie_images(name):
    """ComputeKEY on identical DoG levels: which pixels are extrema (and of which sign) is decided
    by the reference's own comparisons, and must be the oracle's exactly."""
    assert _check_tie_keys(name) > 0
    for (o, j), st in C.levels(name).items():   # the pipeline's key image is the stage's
        assert np.array_equal(_bits(_key_signs(st)), _bits(st["key"])), (o, j)


def _kept(packed):
    """Orientations kept per keypoint from ComputeOrientation's packed float."""
    u = _bits(packed)
    o1, o2 = u & 0xffff, u >> 16
    return np.where(o1 == 65535, 0, np.where((o2 != 65535) & (o2 != o1), 2, 1))


def _packed_angles(packed):
    u = _bits(packed)
    return np.stack([u & 0xffff, u >> 16], 1).astype(np.float64) * (2 * np.pi / 65535.0)


def _angle_diff(a, b):
    return np.abs((a - b + np.pi) % (2 * np.pi) - np.pi)


def _check_tie_orientations(name, max_orientation, pipeline=True):
    n = 0
    for (o, j), st in C.levels(name, max_orientation).items():
        if not len(st["list"]):
            continue
        R.settings(max_orientation=max_orientation)
        try:
            ref = R.orientation(st["list"], st["grad"], st["key"], st["sigma"], st["sigma_step"])
        finally:
            R.settings()
        got = O.stage_orientation(st["list"], st["key"], st["grad"], st["sigma"],
                                  st["sigma_step"], num_orientation=max_orientation)
        if pipeline:   # the pipeline's list after orientation is the stage's
            assert np.array_equal(_bits(got), _bits(st["oriented"])), (o, j)
        if max_orientation == 1:
            assert _angle_diff(ref[:, 3], got[:, 3]).max() <= tol("orientation_angle"), (o, j)
        else:
            assert np.array_equal(_kept(ref[:, 3]), _kept(got[:, 3])), (name, o, j)
            both = _kept(ref[:, 3]) == 2   # two peaks: which is first is a tie decision too
            d = _angle_diff(_packed_angles(ref[:, 3]), _packed_angles(got[:, 3]))
            d[~both, 1] = 0
            d[_kept(ref[:, 3]) == 0] = 0
            assert d.max() <= tol("orientation_angle"), (name, o, j, d.max())
        n += len(got)
    return n


@live
@pytest.mark.parametrize("max_orientation", [2, 1])
@pytest.mark.parametrize("name", list(SI.TIE_IMAGES) + list(C.TIE_ORIENTATION_EXTRA))
def test_orientation_peaks_on_tie_images(name, max_orientation):
    """Which histogram peaks are kept, and in which order, on images whose bins tie exactly: the
    kept count is the reference's for every keypoint and every kept angle is the reference's
    within the float bound (an angle that moved to another equal bin is off by 10 degrees).  The
    two 320 x 240 levels are the ones where equal peak weights occur (tie rules T2 and T4)."""
    assert _check_tie_orientations(name, max_orientation) > 0


# ---- proof that the exact tests bite --------------------------------------------------------

@live
@pytest.mark.parametrize("variant", [1, 6])
def test_key_tie_variants_are_rejected(variant):
    """One extremum tie rule of the oracle flipped (oracle/liboracle_tie<N>.so): the extremum
    test above must fail on checker8."""
    C.levels("checker8")
    with oracle_library(f"liboracle_tie{variant}.so"):
        with pytest.raises(AssertionError):
            _check_tie_keys("checker8")
    _check_tie_keys("checker8")


@live
@pytest.mark.parametrize("variant,max_orientation", [(2, 2), (4, 1)])
def test_orientation_tie_variants_are_rejected(variant, max_orientation):
    """T2 (the two-peak selection replaces on an equal weight) and T4 (the single maximum moves
    to a later equal bin): the orientation test above must fail on checker8 at 320 x 240."""
    name = "checker8@320x240"
    C.levels(name, max_orientation)
    with oracle_library(f"liboracle_tie{variant}.so"):
        with pytest.raises(AssertionError):
            _check_tie_orientations(name, max_orientation, pipeline=False)
    assert _check_tie_orientations(name, max_orientation) > 0


@live
def test_matcher_tie_variant_is_rejected():
    """T7: RowMatch_Kernel's equal maxima given to the lowest column mod 32 -- the rule the oracle
    had until this comparison existed.  The reference's tree reduction keeps thread 8 over thread
    2 (columns 40 and 66), and the tie scenes notice."""
    q1, q2, kw = C.match_case("tie_70x100")
    row, _, _ = R.match_stages(q1, q2, mbm=0, **kw)
    want = R.pairs(row, None)
    with oracle_library("liboracle_tie7.so"):
        bad = _oracle_match(q1, q2, kw, 0)
    assert not np.array_equal(bad, want)
    np.testing.assert_array_equal(_oracle_match(q1, q2, kw, 0), want)
    won = dict(map(tuple, want.tolist()))
    assert 40 in won.values() and 66 not in won.values()


# =============================================================================================
# float stages
# =============================================================================================

@live
@pytest.mark.parametrize("w,h", C.FILTER_SHAPES)
def test_filters(w, h):
    """FilterImage for every sigma of the -d 3 and -d 5 schedules: 16 x 16 (narrower than the
    widest filter), 131 x 37 (three columns past a 128-wide FilterH tile, a partial 128-row
    FilterV tile), 300 x 140 (crosses both tile sizes)."""
    img = C.unit_image(w, h, 3 * w + h)
    a = b = 0.0
    widths = set()
    R.stats()
    c = 0.0
    for sigma in C.filter_sigmas():
        ref = R.filter_image(img, sigma)
        widths.add(len(R.filter_kernel(sigma)))
        got = O.stage_filter(img, sigma)
        a = max(a, float(np.abs(ref - R.filter_image(img, sigma, fast=True)).max()))
        b = max(b, float(np.abs(ref - got).max()))
        c = max(c, float(np.abs(got - _perturbed(lambda: O.stage_filter(img, sigma))).max()))
    assert R.stats()["oob"] == 0
    assert widths >= {9, 11, 13, 15, 17, 21, 25}
    _report("filter", a, b, c)
    assert b <= tol("filter")


@live
def test_filter_taps():
    """CreateFilterKernel is host code of the reference: the oracle's taps, read off the impulse
    response of its filter (the outer product of the taps), have the same width (5 to 33) and
    the same values to a few roundings of exp and of the normalisation."""
    for sigma in C.filter_sigmas() + [0.3, 9.0]:
        ref = R.filter_kernel(sigma)
        img = np.zeros((41, 41), np.float32)
        img[20, 20] = 1.0
        ours = O.stage_filter(img, sigma).astype(np.float64)
        taps = ours[20] / np.sqrt(ours[20, 20])
        half = len(ref) // 2
        assert np.count_nonzero(taps) == len(ref) and 5 <= len(ref) <= 33, sigma
        assert np.abs(taps[20 - half:21 + half] - ref).max() < 3e-7, sigma


@live
def test_octave_change_and_first_octave():
    """SampleImageD at an odd width, SampleImageU, and the byte ingest against the oracle's
    first-octave inputs for -fo 1, 2 and -1."""
    img = C.image("synth_203x97")
    f = R.byte_to_float(img)
    assert np.array_equal(_bits(f), _bits(img.astype(np.float32) / np.float32(255.0)))
    fw = f[:, :200]   # the ingest truncates the width to a multiple of 4
    for fo in (1, 2):
        want = O.first_octave_input(img, fo)
        got = R.sample_d(fw, fo, want.shape[1], want.shape[0])
        assert np.array_equal(_bits(got), _bits(want)), fo
    odd = C.unit_image(131, 37, 5)
    down = R.sample_d(odd, 1, 66, 18)   # column 65 reads min(130, 130)
    assert np.array_equal(down, odd[0:36:2][:, np.minimum(np.arange(66) * 2, 130)])
    want = O.first_octave_input(img, -1)
    R.stats()
    up = R.sample_u(fw, 1)
    oob = R.stats()["oob"]
    a = float(np.abs(up - R.sample_u(fw, 1, fast=True)).max())
    b = float(np.abs(up - want).max())
    c = float(np.abs(want - _perturbed(lambda: O.first_octave_input(img, -1))).max())
    _report("upsample", a, b, c)
    assert oob > 0   # the last row and column blend with fetches past the image: zeros
    assert b <= tol("upsample")


@live
def test_colour_reduce():
    """ReduceToSingleChannel on float RGBA: 0.299 r + 0.587 g + 0.114 b for the four colour
    orders (the caller puts r, g, b in place), and the plain channel pick.  The oracle's colour
    conversion, O.gray_from_color, restates the reference's *host* conversion (GLTexImage.cpp,
    integer weights 19595, 38470, 7471 over 65535), which is what the reference runs by default
    (-prep); this kernel is its -noprep path.  The reference's two formulas differ by their
    weights, sum |w_host - w_kernel| = 1.53e-5 for values in [0, 1]: that, plus the roundings of
    either side, bounds the distance here."""
    weights = sum(abs(a / 65535.0 - b) for a, b in ((19595, 0.299), (38470, 0.587), (7471, 0.114)))
    assert 1.5e-5 < weights < 1.6e-5
    rng = np.random.Generator(np.random.PCG64(11))
    for fmt, c in (("rgb", 3), ("rgba", 4), ("bgr", 3), ("bgra", 4)):
        img = rng.integers(0, 256, (37, 132, c), dtype=np.uint8)
        rgb = img[..., :3] if fmt.startswith("rgb") else img[..., 2::-1]
        rgba = np.concatenate([rgb, np.full((37, 132, 1), 255, np.uint8)], 2).astype(np.float32)
        rgba /= np.float32(255.0)
        ref = R.reduce_channel(rgba, True)
        exact = (0.299 * rgba[..., 0].astype(np.float64) + 0.587 * rgba[..., 1] + 0.114 * rgba[..., 2])
        assert np.abs(ref - exact).max() < 2.0 ** -23
        assert np.abs(ref - O.gray_from_color(img, fmt)).max() <= weights + 2.0 ** -22
        assert np.array_equal(R.reduce_channel(rgba, False), rgba[..., 0])


@live
@pytest.mark.parametrize("name", sorted(C.FLOAT_IMAGES))
def test_gradient(name):
    am = bm = cm = aa = ba = ca = 0.0
    oob = 0
    for (o, j), st in C.levels(name).items():
        h, wa = st["dog"].shape[1:]
        g = [O.gaussian(C.image(name), o, m).reshape(h, wa) for m in (j, j + 1)]
        R.stats()
        ref = R.dog(g[0], g[1], True)[1]
        oob += R.stats()["oob"]
        fast = R.dog(g[0], g[1], True, fast=True)[1]
        got = O.stage_dog(g[0], g[1], True)[1]
        per = _perturbed(lambda: O.stage_dog(g[0], g[1], True)[1])
        assert np.array_equal(_bits(got), _bits(st["grad"]))
        am = max(am, float(np.abs(ref[..., 0] - fast[..., 0]).max()))
        bm = max(bm, float(np.abs(ref[..., 0] - got[..., 0]).max()))
        cm = max(cm, float(np.abs(got[..., 0] - per[..., 0]).max()))
        # the angle is compared on the circle: -pi and pi are one direction
        aa = max(aa, float(_angle_diff(ref[..., 1], fast[..., 1]).max()))
        ba = max(ba, float(_angle_diff(ref[..., 1], got[..., 1]).max()))
        ca = max(ca, float(_angle_diff(got[..., 1], per[..., 1]).max()))
    _report("gradient_magnitude", am, bm, cm)
    _report("gradient_angle", aa, ba, ca)
    assert oob > 0   # the first and last rows fetch past the level: zeros, as the oracle has it
    assert bm <= tol("gradient_magnitude") and ba <= tol("gradient_angle")


@live
@pytest.mark.parametrize("name", sorted(C.FLOAT_IMAGES))
def test_key_offsets_and_scales(name):
    """ComputeKEY's candidate sets and sub-pixel offsets, and the scale ComputeOrientation
    derives from the offset (sigma * sigma_step ^ ds, a pow)."""
    a = b = c = 0.0
    sa = sb = sc = 0.0
    union = differ = 0
    for (o, j), st in C.levels(name).items():
        ref, fast, got = _key_signs(st, False), _key_signs(st, False, True), _key_signs(st)
        per = _perturbed(lambda: _key_signs(st))
        assert np.array_equal(per[..., 0], got[..., 0])
        for other in (fast, got):
            sel = (ref[..., 0] != 0) | (other[..., 0] != 0)
            union += int(sel.sum())
            differ += int((ref[..., 0] != other[..., 0]).sum())
        both = (ref[..., 0] != 0) & (got[..., 0] != 0) & (fast[..., 0] != 0)
        if both.any():
            a = max(a, float(np.abs(ref[both, 1:] - fast[both, 1:]).max()))
            b = max(b, float(np.abs(ref[both, 1:] - got[both, 1:]).max()))
            c = max(c, float(np.abs(per[both, 1:] - got[both, 1:]).max()))
        if len(st["list"]):
            r = R.orientation(st["list"], st["grad"], st["key"], st["sigma"], st["sigma_step"])
            f = R.orientation(st["list"], st["grad"], st["key"], st["sigma"], st["sigma_step"], fast=True)
            q = O.stage_orientation(st["list"], st["key"], st["grad"], st["sigma"], st["sigma_step"])
            p = _perturbed(lambda: O.stage_orientation(st["list"], st["key"], st["grad"],
                                                       st["sigma"], st["sigma_step"]))
            assert np.array_equal(_bits(r[:, :2]), _bits(q[:, :2]))   # x, y: one addition
            sa = max(sa, float(np.abs(r[:, 2] / f[:, 2] - 1).max()))
            sb = max(sb, float(np.abs(r[:, 2] / q[:, 2] - 1).max()))
            sc = max(sc, float(np.abs(p[:, 2] / q[:, 2] - 1).max()))
    _report("key_offset", a, b, c)
    _report("key_scale_rel", sa, sb, sc)
    # set-valued: no more than 1 % of the union may differ (none does on these images, between
    # the two contraction builds or against the oracle)
    assert differ <= 0.01 * union and union > 100
    assert differ == 0
    assert b <= tol("key_offset") and sb <= tol("key_scale_rel")


def _border_keys(w, h):
    """Keypoints within one descriptor radius of each border and corner (scale 2, 3 bins of 3
    scale units each side)."""
    pts = [(3.0, h / 2), (w - 3.0, h / 2), (w / 2, 3.0), (w / 2, h - 3.0), (2.5, 2.5),
           (w - 2.5, h - 2.5), (w / 2, h / 2)]
    return np.array([[x, y, 2.0, 0.7 * i] for i, (x, y) in enumerate(pts)], np.float32)


@live
@pytest.mark.parametrize("name", sorted(C.FLOAT_IMAGES))
def test_orientation_angles_and_descriptors(name):
    img = C.image(name)
    feat, lvl = O.features_oct(img)
    ao = bo = co = 0.0
    m = {k: [0.0, 0.0, 0.0] for k in ("descriptor_l2", "descriptor_unnormalized_rel",
                                      "descriptor_rect_l2")}
    kept_union = kept_differ = 0
    for (o, j), st in C.levels(name).items():
        h, wa = st["grad"].shape[:2]
        if len(st["list"]):
            args = (st["list"], st["grad"], st["key"], st["sigma"], st["sigma_step"])
            r, f = R.orientation(*args), R.orientation(*args, fast=True)
            q = O.stage_orientation(st["list"], st["key"], st["grad"], st["sigma"], st["sigma_step"])
            p = _perturbed(lambda: O.stage_orientation(st["list"], st["key"], st["grad"],
                                                       st["sigma"], st["sigma_step"]))
            kept_union += 2 * len(q)
            kept_differ += int((_kept(r[:, 3]) != _kept(q[:, 3])).sum()) + \
                int((_kept(r[:, 3]) != _kept(f[:, 3])).sum())
            same = (_kept(r[:, 3]) == _kept(q[:, 3])) & (_kept(r[:, 3]) == _kept(f[:, 3])) & \
                (_kept(p[:, 3]) == _kept(q[:, 3]))
            mask = np.stack([_kept(q[:, 3]) >= 1, _kept(q[:, 3]) == 2], 1) & same[:, None]
            ang = [_packed_angles(v[:, 3]) for v in (r, f, q, p)]
            if mask.any():
                ao = max(ao, float(_angle_diff(ang[0], ang[1])[mask].max()))
                bo = max(bo, float(_angle_diff(ang[0], ang[2])[mask].max()))
                co = max(co, float(_angle_diff(ang[3], ang[2])[mask].max()))
        keys = np.concatenate([feat[lvl == o * 3 + j], _border_keys(wa, h)])
        for window, normalized, rect, what in ((3.0, 1, False, "descriptor_l2"),
                                               (2.0, 1, False, "descriptor_l2"),
                                               (3.0, 0, False, "descriptor_unnormalized_rel"),
                                               (3.0, 1, True, "descriptor_rect_l2"),
                                               (3.0, 0, True, "descriptor_unnormalized_rel")):
            k = keys.copy()
            if rect:   # (x, y, width, height) rectangles around the same points
                k[:, 2:] = 12.0 * keys[:, 2:3]
                k[:, :2] -= 6.0 * keys[:, 2:3]
            for fast in (False, True):
                R.settings(fast=fast, descriptor_window_factor=window, normalized=normalized,
                           dynamic_indexing=0)
            try:
                r = R.descriptor(k, st["grad"], rect)
                f = R.descriptor(k, st["grad"], rect, fast=True)
                R.settings(descriptor_window_factor=window, normalized=normalized,
                           dynamic_indexing=1)
                assert np.array_equal(_bits(R.descriptor(k, st["grad"], rect)), _bits(r))
            finally:
                R.settings()
                R.settings(fast=True)
            q = O.stage_descriptor(k, st["grad"], window, normalized, rect)
            p = _perturbed(lambda: O.stage_descriptor(k, st["grad"], window, normalized, rect))
            scale = 1.0 if normalized else np.maximum(np.linalg.norm(r, axis=1), 1e-12)
            for i, (x, y) in enumerate(((r, f), (r, q), (p, q))):
                m[what][i] = max(m[what][i], float((np.linalg.norm(x - y, axis=1) / scale).max()))
    _report("orientation_angle", ao, bo, co)
    for what, v in m.items():
        _report(what, *v)
    # set-valued: the kept count differs for no keypoint of these images, between the two
    # contraction builds or against the oracle, so no element needs a margin shown
    assert kept_differ == 0 and kept_union > 100
    assert bo <= tol("orientation_angle")
    for what, v in m.items():
        assert v[1] <= tol(what), what


# =============================================================================================
# fixtures: the pin holds without the reference
# =============================================================================================

def _golden(name):
    path = os.path.join(GOLDEN, name)
    assert os.path.exists(path), f"{name} missing (tests/make_ref_golden.py)"
    return np.load(path)


def _close_recorded(live_value, recorded):
    """Float stages: within one rounding of the recorded float32 (libm differs by machine)."""
    a = np.asarray(live_value, np.float32).astype(np.float64)
    b = np.asarray(recorded, np.float32).astype(np.float64)
    return np.all(np.abs(a - b) <= np.spacing(np.abs(recorded).astype(np.float32)))


def test_fixture_matcher():
    z = _golden("ref_match.npz")
    for name in C.MATCH_SMALL:
        q1, q2, kw = C.match_case(name)
        for mbm in (0, 1):
            np.testing.assert_array_equal(_oracle_match(q1, q2, kw, mbm), z[f"{name}_mbm{mbm}"])
            if R.available():
                row, col, _ = R.match_stages(q1, q2, mbm=mbm, **kw)
                np.testing.assert_array_equal(R.pairs(row, col), z[f"{name}_mbm{mbm}"])
    for name in C.GUIDED_SMALL:
        np.testing.assert_array_equal(_guided(name, _oracle_guided), z[f"guided_{name}"])
        if R.available():
            np.testing.assert_array_equal(_guided(name, _ref_guided), z[f"guided_{name}"])
    assert list(C.guided_case("block_rule")[6]["planted"]) in z["guided_block_rule"].tolist()


def test_fixture_tie_image_keys():
    """checker8's extremum decisions, first octave: the recorded sign images of ComputeKEY."""
    z = _golden("ref_keys_checker8.npz")
    total = 0
    for j in range(3):
        st = C.levels("checker8")[(0, j)]
        signs = z[f"sign_{j}"]
        total += int(np.count_nonzero(signs))
        assert np.array_equal(_key_signs(st)[..., 0].astype(np.int8), signs), j
        if R.available():
            assert np.array_equal(_key_signs(st, False)[..., 0].astype(np.int8), signs), j
    assert total == 186   # tests/test_structured_images.py COUNTS_203 has the same candidates


def test_fixture_filters():
    z = _golden("ref_filter.npz")
    img = C.unit_image(131, 37, 3 * 131 + 37)
    seen = set()
    for i, sigma in enumerate(z["sigmas"]):
        rec = z[f"level_{i}"]
        seen.add(int(z["widths"][i]))
        assert np.abs(O.stage_filter(img, float(sigma)) - rec).max() <= tol("filter")
        if R.available():
            assert _close_recorded(R.filter_image(img, float(sigma)), rec)
    assert seen == {9, 11, 13, 15, 17, 21, 25}


def test_fixture_features_160x120():
    """Keys, packed orientations and every descriptor of synth_image(160, 120, 1),
    every level of two octaves, as the reference's kernels gave them on the oracle's inputs."""
    z = _golden("ref_features_160x120.npz")
    feat, lvl = O.features_oct(C.image("synth_160x120"))
    n = 0
    for (o, j), st in C.levels("synth_160x120").items():
        rec = z[f"oriented_{o}_{j}"]
        got = O.stage_orientation(st["list"], st["key"], st["grad"], st["sigma"], st["sigma_step"])
        assert np.array_equal(_bits(got[:, :2]), _bits(rec[:, :2]))
        assert np.abs(got[:, 2] / rec[:, 2] - 1).max() <= tol("key_scale_rel") if len(rec) else True
        assert np.array_equal(_kept(got[:, 3]), _kept(rec[:, 3]))
        d = _angle_diff(_packed_angles(got[:, 3]), _packed_angles(rec[:, 3]))
        d[_kept(rec[:, 3]) < 2, 1] = 0
        d[_kept(rec[:, 3]) == 0] = 0
        assert d.size == 0 or d.max() <= tol("orientation_angle")
        keys = feat[lvl == o * 3 + j]
        recd = z[f"desc_{o}_{j}"]
        gotd = O.stage_descriptor(keys, st["grad"])
        assert len(recd) == len(keys)
        if len(keys):
            assert np.linalg.norm(gotd - recd, axis=1).max() <= tol("descriptor_l2")
        n += len(keys)
        if R.available():
            assert _close_recorded(R.descriptor(keys, st["grad"]), recd)
            live_o = R.orientation(st["list"], st["grad"], st["key"], st["sigma"], st["sigma_step"])
            assert _close_recorded(live_o[:, :3], rec[:, :3])
            assert np.array_equal(_kept(live_o[:, 3]), _kept(rec[:, 3]))
    assert n > 100
