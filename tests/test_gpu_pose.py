"""sgpu_pose_batch / sgpu_pose_images: relative pose and triangulation of verified pairs on the device.

Expected values never come from the library: they are spose::pose_host's (csrc/sift_pose.h), run by
the stand-alone program tests/abi/pose_check.cpp, built plain with g++ at test time.  The device's
R, t and points (as bytes), counts and masks must be identical to it; a mismatch is a finding in
the operation order, there is no tolerance.  What pose_host computes is pinned on the CPU by
test_pose.py against a NumPy float64 reference and the planted motion.

 1  the edge-pair list of pose_scenes.pair_list, also at f_threshold 1e20 and other angles;
 2  m = 1, 63, 64, 65, 129 with the non-participants at lanes 0 and 63;
 3  3,000 eight-match filler pairs around the real ones; the repeated call allocates nothing;
 4  out_mask / out_points NULL in every combination; device-resident locations;
 5  pose_images after an extract equals pose_batch on the downloaded keys, also on a two-part batch;
 6  times[16] is the call's, slots 0-15 stay; every SGPU_EINVAL case leaves the outputs untouched."""
import functools

import numpy as np
import pytest

import pose_scenes as S
import sgpu
from sgpu_types import default_options
from sift_synth import synth_image

gpu = pytest.mark.gpu


def _same(got, want):
    for name in ("R", "t"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape and g.dtype == w.dtype == np.float32, name
        bad = [p for p in range(len(w)) if g[p].tobytes() != w[p].tobytes()]
        assert not bad, (name, bad[:8], g[bad[0]], w[bad[0]])
    for name in ("participants", "front", "wide"):
        assert getattr(got, name).tolist() == getattr(want, name).tolist(), name
    assert len(got.masks) == len(want.masks) == len(got.points) == len(want.points)
    for p, (a, b) in enumerate(zip(got.masks, want.masks)):
        assert a.dtype == bool and np.array_equal(a, b), p
    for p, (a, b) in enumerate(zip(got.points, want.points)):
        assert a.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes(), p


@functools.lru_cache(maxsize=None)
def _host(which, threshold=S.THRESHOLD, min_angle=S.MIN_ANGLE):
    pl = {"edge": S.pair_list, "lanes": S.lane_list, "fill": S.filler_list}[which]()
    return S.host_pose(*pl, threshold=threshold, min_angle=min_angle)


def _device(gpu_ctx, pl, threshold=S.THRESHOLD, min_angle=S.MIN_ANGLE, **kw):
    return gpu_ctx.pose_batch(pl.loc, pl.off, pl.pairs, pl.matches, pl.F, pl.K, threshold, min_angle, **kw)


# ---- 1: the planted scene and the edge pairs ---------------------------------------------------------

@gpu
def test_planted_scene_and_edge_pairs(gpu_ctx):
    """pose_scenes.pair_list: the scene, an empty pair between real ones, (b, a) under F', the
    repeat, m = 0, parallel rays, a zero, a rank-1 and a NaN F, an empty set; set 0 starts at
    buffer row 5."""
    pl = S.pair_list()
    want = _host("edge")
    assert pl.off[0] == 5 and want.candidates[0].tolist() == [0, 129, 0, 0]
    assert want.front.tolist() == [129, 0, 129, 129, 0, 0, 0, 0, 0, 0] and 0 < want.wide[0] < 129
    assert want.participants[5] == 10 and not want.R[5].any()
    got = _device(gpu_ctx, pl)
    _same(got, want)
    assert got.R[3].tobytes() == got.R[0].tobytes() and got.points[3].tobytes() == got.points[0].tobytes()


@gpu
@pytest.mark.parametrize("threshold,min_angle", [(1e20, S.MIN_ANGLE), (4.0, 0.0), (0.0, 0.1),
                                                 (4.0, float(np.float32(np.pi / 2)))])
def test_thresholds_and_angles(gpu_ctx, threshold, min_angle):
    want = _host("edge", threshold, min_angle)
    if threshold == 1e20:
        assert want.participants[7] == 129        # every match, also under the rank-1 F
    if min_angle == 0.0:
        assert want.wide.tolist() == want.front.tolist()
    if min_angle > 1.5:
        assert not want.wide.any()
    _same(_device(gpu_ctx, S.pair_list(), threshold, min_angle), want)


# ---- 2: the lane stride -----------------------------------------------------------------------------

@gpu
def test_lane_stride_boundaries(gpu_ctx):
    want = _host("lanes")
    for p, m in enumerate(S.LANE_COUNTS):
        edge = np.isin(np.arange(m) % 64, (0, 63))
        assert want.participants[p] == m - edge.sum() == want.front[p], (p, m)
        assert not want.masks[p][edge].any() and want.masks[p][~edge].all()
    assert want.participants.tolist() == [0, 62, 62, 62, 124]
    _same(_device(gpu_ctx, S.lane_list()), want)
    # one pair at a time: the same results, whatever the list around a pair
    pl = S.lane_list()
    for p in (0, 3):
        one = gpu_ctx.pose_batch(pl.loc, pl.off, pl.pairs[p:p + 1], pl.matches[p:p + 1], pl.F[p:p + 1],
                                 pl.K, S.THRESHOLD, S.MIN_ANGLE)
        assert one.R[0].tobytes() == want.R[p].tobytes() and np.array_equal(one.masks[0], want.masks[p])
        assert one.points[0].tobytes() == want.points[p].tobytes()


# ---- 3: launch independence --------------------------------------------------------------------------

@gpu
def test_launch_independence_and_allocations(gpu_ctx):
    pl = S.filler_list()
    want = _host("fill")
    first = _host("edge")
    for p in S.REAL:
        assert want.front[p] == 129 and want.R[p].tobytes() == first.R[0].tobytes()
    assert want.participants[1] == 8 and want.front[2000] == 8
    got = _device(gpu_ctx, pl)
    _same(got, want)
    before = gpu_ctx.alloc_count()
    _same(_device(gpu_ctx, pl), want)
    _same(_device(gpu_ctx, S.pair_list()), first)      # a smaller shape fits too
    assert gpu_ctx.alloc_count() == before


# ---- 4: optional outputs, device-resident locations ----------------------------------------------------

def _c_call(gpu_ctx, pl, threshold=S.THRESHOLD, min_angle=S.MIN_ANGLE, mask=True, points=True,
            loc_ptr=None, flags=sgpu.SGPU_INPUT_HOST, nsets=None, **null):
    """The C call with arrays prefilled with 7: (rc, {name: array})."""
    pr = np.ascontiguousarray(pl.pairs, np.int32).reshape(-1, 2)
    ms = [np.ascontiguousarray(m, np.int32).reshape(-1, 2) for m in pl.matches]
    mt = np.ascontiguousarray(np.concatenate(ms + [np.zeros((0, 2), np.int32)]), np.int32)
    ct = np.array([len(m) for m in ms], np.int32)
    lc = np.ascontiguousarray(pl.loc, np.float32)
    of = np.ascontiguousarray(pl.off, np.int64)
    K = np.ascontiguousarray(pl.K, np.float32)
    F = np.ascontiguousarray(pl.F, np.float32).reshape(-1, 9)
    outs = dict(R=np.full((len(pr), 9), 7, np.float32), t=np.full((len(pr), 3), 7, np.float32),
                counts=np.full((len(pr), 3), 7, np.int32), mask=np.full(max(len(mt), 1), 7, np.uint8),
                points=np.full((max(len(mt), 1), 3), 7, np.float32))
    arg = lambda name, a: None if null.get(name) else a.ctypes.data
    rc = sgpu.lib().sgpu_pose_batch(
        gpu_ctx._ctx, loc_ptr if loc_ptr is not None else arg("loc", lc), arg("off", of),
        len(of) - 1 if nsets is None else nsets, arg("K", K), arg("pairs", pr), len(pr),
        arg("matches", mt), arg("match_counts", ct), arg("F", F), threshold, min_angle,
        arg("R", outs["R"]), arg("t", outs["t"]), arg("counts", outs["counts"]),
        outs["mask"].ctypes.data if mask else None, outs["points"].ctypes.data if points else None, flags)
    return rc, outs


def _untouched(outs):
    return all((a == 7).all() for a in outs.values())


def _check_outs(outs, want, mask, points):
    n = len(want.R)
    assert outs["R"].tobytes() == want.R.tobytes() and outs["t"].tobytes() == want.t.tobytes()
    assert outs["counts"].tolist() == np.stack([want.participants, want.front, want.wide], 1).tolist()
    if mask:
        assert np.array_equal(outs["mask"].astype(bool), np.concatenate(want.masks))
    else:
        assert (outs["mask"] == 7).all()
    if points:
        assert outs["points"].tobytes() == np.concatenate(want.points).tobytes()
    else:
        assert (outs["points"] == 7).all()
    assert n == len(outs["counts"])


@gpu
@pytest.mark.parametrize("mask,points", [(True, True), (True, False), (False, True), (False, False)])
def test_optional_outputs(gpu_ctx, mask, points):
    rc, outs = _c_call(gpu_ctx, S.pair_list(), mask=mask, points=points)
    assert rc == sgpu.SGPU_OK
    _check_outs(outs, _host("edge"), mask, points)


@gpu
def test_device_resident_locations(gpu_ctx):
    """SGPU_INPUT_DEVICE: the locations are read in place, 8 bytes into an allocation."""
    import devmem
    pl = S.pair_list()
    with devmem.uploaded(pl.loc, offset=8) as addr:
        got = gpu_ctx.pose_batch(None, pl.off, pl.pairs, pl.matches, pl.F, pl.K, S.THRESHOLD,
                                 S.MIN_ANGLE, device_ptr=addr)
        _same(got, _host("edge"))
        rc, outs = _c_call(gpu_ctx, pl, points=False, loc_ptr=addr, flags=sgpu.SGPU_INPUT_DEVICE)
    assert rc == sgpu.SGPU_OK
    _check_outs(outs, _host("edge"), True, False)
    none = gpu_ctx.pose_batch(pl.loc, pl.off, pl.pairs, pl.matches, pl.F, pl.K, points=False)
    assert none.points is None and none.front.tolist() == _host("edge").front.tolist()


# ---- 5: over an extracted batch -------------------------------------------------------------------------

ROLLS = [(0, 0), (7, 11)]   # (rows, columns) each view is rolled by
IMAGE_PAIRS = [(0, 1), (1, 0), (0, 1)]
IMAGE_K = np.array([(300.0, 310.0, 160.0, 120.0), (280.0, 285.0, 150.0, 125.0)], np.float32)


def _views():
    img = synth_image(320, 240, 55)
    return np.stack([np.roll(img, s, axis=(0, 1)) for s in ROLLS])


def _check_images(gpu_ctx):
    plain = gpu_ctx.match_images(IMAGE_PAIRS)
    assert min(len(m) for m in plain) > 50
    F, inliers, _ = gpu_ctx.estimate_images(IMAGE_PAIRS, plain, "F", 4.0, 256, 5)
    assert (inliers > 20).all()
    F[2] = 0                                      # a pair without a model
    got = gpu_ctx.pose_images(IMAGE_PAIRS, plain, F, IMAGE_K, 4.0, S.MIN_ANGLE)
    keys = [np.ascontiguousarray(gpu_ctx.features(i, descriptors=False)[0][:, :2], np.float32)
            for i in range(2)]
    off = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)
    loc = np.concatenate(keys)
    batch = gpu_ctx.pose_batch(loc, off, IMAGE_PAIRS, plain, F, IMAGE_K, 4.0, S.MIN_ANGLE)
    _same(got, batch)
    _same(batch, S.host_pose(loc, off, IMAGE_K, IMAGE_PAIRS, plain, F, 4.0, S.MIN_ANGLE))
    assert got.participants[0] >= inliers[0] > 0 and got.participants[2] == 0
    assert not got.R[2].any()


@gpu
def test_pose_images_equals_pose_batch(gpu_ctx):
    gpu_ctx.set_options(default_options())
    views = _views()
    gpu_ctx.extract(views)
    _check_images(gpu_ctx)
    with pytest.raises(RuntimeError):
        gpu_ctx.pose_images([(0, 2)], [np.zeros((0, 2), np.int32)], np.zeros((1, 3, 3)), IMAGE_K)
    with pytest.raises(RuntimeError):   # a match index outside image 1's features
        gpu_ctx.pose_images([(0, 1)], [np.array([[0, gpu_ctx.count(1)]], np.int32)],
                            np.zeros((1, 3, 3)), IMAGE_K)
    try:
        gpu_ctx.set_debug_flags(gpu_ctx.DEBUG_PARTS2)
        gpu_ctx.extract(views)
        _check_images(gpu_ctx)
    finally:
        gpu_ctx.set_debug_flags(0)


# ---- 6: timing, errors ------------------------------------------------------------------------------------

def _times(gpu_ctx, n=17):
    t = np.full(n, -1.0, np.float32)
    assert sgpu.lib().sgpu_last_timing(gpu_ctx._ctx, t.ctypes.data, n) == sgpu.SGPU_OK
    return t


@gpu
def test_timing_slot(gpu_ctx):
    pl = S.pair_list()
    _device(gpu_ctx, pl)
    before = _times(gpu_ctx)
    _device(gpu_ctx, pl)
    after = _times(gpu_ctx)
    assert after[16] > 0 and gpu_ctx.pose_time() == after[16]
    assert np.array_equal(after[:16], before[:16])
    assert _times(gpu_ctx, 20)[17:].tolist() == [-1.0] * 3
    assert len(gpu_ctx.timing()) == 10


@gpu
def test_bad_arguments_leave_the_outputs_untouched(gpu_ctx):
    pl = S.lane_list()
    rc, outs = _c_call(gpu_ctx, pl)
    assert rc == sgpu.SGPU_OK and not _untouched(outs)
    nan, inf = float("nan"), float("inf")

    def with_K(row, col, v):
        K = pl.K.copy()
        K[row, col] = v
        return pl._replace(K=K)

    def with_match(i, j):
        ms = [m.copy() for m in pl.matches]
        ms[1][5] = (i, j)
        return pl._replace(matches=ms)

    n0 = int(pl.off[1] - pl.off[0])
    n1 = int(pl.off[2] - pl.off[1])
    bad = [(pl, dict(threshold=-1.0)), (pl, dict(threshold=nan)), (pl, dict(threshold=inf)),
           (pl, dict(min_angle=-0.01)), (pl, dict(min_angle=1.6)), (pl, dict(min_angle=nan)),
           (pl, dict(F=True)), (pl, dict(K=True)), (pl, dict(R=True)), (pl, dict(t=True)),
           (pl, dict(counts=True)), (pl, dict(matches=True)), (pl, dict(match_counts=True)),
           (pl, dict(pairs=True)), (pl, dict(off=True)), (pl, dict(loc=True)), (pl, dict(nsets=-1)),
           (pl._replace(pairs=[(0, 2)] + pl.pairs[1:]), {}), (pl._replace(pairs=[(-1, 1)] + pl.pairs[1:]), {}),
           (pl._replace(off=np.array([0, n0, n0 - 1], np.int64)), {}),
           (with_match(n0, 0), {}), (with_match(0, n1), {}), (with_match(-1, 0), {}),
           (with_K(0, 0, 0.0), {}), (with_K(1, 1, -600.0), {}), (with_K(0, 2, nan), {}),
           (with_K(1, 3, inf), {}), (with_K(1, 0, inf), {})]
    for case, kw in bad:
        rc, outs = _c_call(gpu_ctx, case, **kw)
        assert rc == sgpu.SGPU_EINVAL, kw
        assert _untouched(outs), kw
        assert sgpu.lib().sgpu_last_error(gpu_ctx._ctx), kw
    # the intrinsics of a set that no pair names may hold anything
    three = pl._replace(off=np.r_[pl.off, pl.off[-1]], K=np.r_[pl.K, [[nan, -1, inf, 0]]].astype(np.float32))
    rc, outs = _c_call(gpu_ctx, three)
    assert rc == sgpu.SGPU_OK
    _check_outs(outs, _host("lanes"), True, True)
    # no pairs: nothing to write, nothing needed
    empty = gpu_ctx.pose_batch(pl.loc, pl.off, [], [], np.zeros((0, 3, 3), np.float32), pl.K)
    assert empty.R.shape == (0, 3, 3) and empty.masks == [] and empty.points == []
    with pytest.raises(RuntimeError):
        gpu_ctx.pose_batch(pl.loc, pl.off, [(0, 5)], [pl.matches[0]], pl.F[:1], pl.K)
    _same(_device(gpu_ctx, pl), _host("lanes"))       # the context still works
