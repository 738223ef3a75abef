"""sgpu_estimate_batch_refined / sgpu_estimate_images_refined: the estimator's winner refitted on
its inliers, on the device.

Expected values never come from the library: they are sgeo::refine_host's (csrc/sift_geom.h), run
by the stand-alone program tests/abi/geom_refine_check.cpp, built plain with g++ at test time.  The
device's models (as bytes), inlier counts, masks and accepted rounds must be bit-identical to it; a
mismatch is a finding in the operation order, there is no tolerance.  What refine_host computes is
pinned on the CPU by test_geom_refine.py."""
import functools

import numpy as np
import pytest

import geom_refine_scenes as R
import geom_scenes as G
import sgpu
from sgpu_types import default_options
from sift_synth import synth_image

gpu = pytest.mark.gpu
CASES = {"H": G.H_CASE, "F": G.F_CASE}
TIGHT = {"H": R.H_TIGHT, "F": R.F_TIGHT}


def _same(got, want):
    gm, gi, gk, gr = got
    wm, wi, wk, wr = want
    assert gm.shape == wm.shape and gm.dtype == wm.dtype == np.float32
    bad = [p for p in range(len(wm)) if gm[p].tobytes() != wm[p].tobytes()]
    assert not bad, (bad[:8], gm[bad[0]], wm[bad[0]])
    assert gi.tolist() == wi.tolist()
    assert gr.dtype == np.int32 and gr.tolist() == wr.tolist()
    assert len(gk) == len(wk)
    for p, (a, b) in enumerate(zip(gk, wk)):
        assert a.dtype == bool and np.array_equal(a, b), p


@functools.lru_cache(maxsize=None)
def _host(model, rounds, tight=False):
    loc, off, pairs, matches, _ = G.pair_list(model)
    return R.host_refine(loc, off, pairs, matches, rounds=rounds, **(TIGHT if tight else CASES)[model])


# ---- 1: the planted scenes and the edge pairs, every round budget ---------------------------------

@gpu
@pytest.mark.parametrize("rounds", [0, 1, 3, 8])
@pytest.mark.parametrize("model", ["H", "F"])
def test_planted_scenes_and_edge_pairs(gpu_ctx, model, rounds):
    """geom_scenes.pair_list: the scene, the pairs without a model, m = S - 1, S, S + 1, the pair
    at one point.  rounds = 0: also the unrefined call's bytes."""
    loc, off, pairs, matches, _ = G.pair_list(model)
    want = _host(model, rounds)
    assert (want[3] > 0).any() == (rounds > 0) and not want[3][[1, 4, 5, 8, 9]].any()
    got = gpu_ctx.estimate_batch_refined(loc, off, pairs, matches, rounds=rounds, **CASES[model])
    _same(got, want)
    if rounds == 0:
        plain = gpu_ctx.estimate_batch(loc, off, pairs, matches, **CASES[model])
        _same(got, plain + (np.zeros(len(pairs), np.int32),))


@gpu
@pytest.mark.parametrize("model", ["H", "F"])
def test_tight_thresholds(gpu_ctx, model):
    """H at 0.45 px and F at 0.15 px^2, 8 rounds: several accepted rounds, the gain in inliers, and
    (F, positions 0 and 2) a rejected round."""
    loc, off, pairs, matches, _ = G.pair_list(model)
    want = _host(model, 8, True)
    plain = G.host_estimate(loc, off, pairs, matches, **TIGHT[model])
    assert want[3].max() >= 2 and (want[1][[0, 2, 3]] - plain[1][[0, 2, 3]]).min() >= (5 if model == "H" else 25)
    _same(gpu_ctx.estimate_batch_refined(loc, off, pairs, matches, rounds=8, **TIGHT[model]), want)


# ---- 2: the partial sums' lane edges ----------------------------------------------------------------

@gpu
@pytest.mark.parametrize("m", [63, 64, 65, 129])
def test_lane_edges(gpu_ctx, m):
    la, lb, mt, _ = G.h_scene(seed=320 + (m % 7), n=m, n_planted=(3 * m) // 5)
    loc = np.concatenate([la, lb])
    off = np.array([0, m, 2 * m], np.int64)
    want = R.host_refine(loc, off, [(0, 1)], [mt], rounds=3, **G.H_CASE)
    assert want[3][0] >= 1
    _same(gpu_ctx.estimate_batch_refined(loc, off, [(0, 1)], [mt], rounds=3, **G.H_CASE), want)


# ---- 3: launch independence, repeated shapes --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _filler_list():
    """300 filler pairs of m = 4 (the first four planted matches) with the scene at positions 0,
    63, 64 and last."""
    loc, off, pairs, matches, planted = G.pair_list("H")
    fill = matches[0][planted][:4]
    real = [0, 63, 64, 303]
    ps = [(0, 1)] * 304
    ms = [matches[0] if p in real else fill for p in range(304)]
    return loc, off, ps, ms, real


@gpu
def test_launch_independence(gpu_ctx):
    loc, off, ps, ms, real = _filler_list()
    want = R.host_refine(loc, off, ps, ms, rounds=3, **R.H_TIGHT)
    assert all(want[3][p] >= 1 for p in real)
    got = gpu_ctx.estimate_batch_refined(loc, off, ps, ms, rounds=3, **R.H_TIGHT)
    _same(got, want)
    # position 0 is the stand-alone list's position 0, whatever follows it
    first = _host("H", 3, True)
    assert got[0][0].tobytes() == first[0][0].tobytes() and np.array_equal(got[2][0], first[2][0])
    assert got[1][0] == first[1][0] and got[3][0] == first[3][0]
    before = gpu_ctx.alloc_count()
    _same(gpu_ctx.estimate_batch_refined(loc, off, ps, ms, rounds=3, **R.H_TIGHT), want)
    assert gpu_ctx.alloc_count() == before


@gpu
def test_device_resident_locations(gpu_ctx):
    """SGPU_INPUT_DEVICE: the locations are read in place, 8 bytes into an allocation."""
    import devmem
    loc, off, pairs, matches, _ = G.pair_list("F")
    with devmem.uploaded(loc, offset=8) as addr:
        got = gpu_ctx.estimate_batch_refined(None, off, pairs, matches, rounds=3, device_ptr=addr,
                                             **G.F_CASE)
    _same(got, _host("F", 3))


# ---- 4: the C interface ------------------------------------------------------------------------------

def _c_call(gpu_ctx, rounds, out_rounds=True, mask=True):
    loc, off, pairs, matches, _ = G.pair_list("H")
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    mt = np.ascontiguousarray(np.concatenate(matches), np.int32)
    ct = np.array([len(m) for m in matches], np.int32)
    lc = np.ascontiguousarray(loc, np.float32)
    of = np.ascontiguousarray(off, np.int64)
    om = np.zeros((len(pr), 9), np.float32)
    oi = np.zeros(len(pr), np.int32)
    ok = np.zeros(len(mt), np.uint8)
    done = np.full(len(pr), -7, np.int32)
    rc = sgpu.lib().sgpu_estimate_batch_refined(
        gpu_ctx._ctx, lc.ctypes.data, of.ctypes.data, len(of) - 1, pr.ctypes.data, len(pr),
        mt.ctypes.data, ct.ctypes.data, 0, G.H_CASE["threshold"], G.H_CASE["iterations"],
        G.H_CASE["seed"], rounds, om.ctypes.data, oi.ctypes.data, ok.ctypes.data if mask else None,
        done.ctypes.data if out_rounds else None, sgpu.SGPU_INPUT_HOST)
    return rc, om.reshape(-1, 3, 3), oi, ok, done


def _times(gpu_ctx, n=13):
    t = np.full(n, -1.0, np.float32)
    assert sgpu.lib().sgpu_last_timing(gpu_ctx._ctx, t.ctypes.data, n) == sgpu.SGPU_OK
    return t


@gpu
def test_round_range_null_outputs_and_timing(gpu_ctx):
    want = _host("H", 3)
    before = _times(gpu_ctx)
    rc, om, oi, ok, done = _c_call(gpu_ctx, 3)
    after = _times(gpu_ctx)
    assert rc == sgpu.SGPU_OK and om.tobytes() == want[0].tobytes() and oi.tolist() == want[1].tolist()
    assert done.tolist() == want[3].tolist() and ok.tolist() == np.concatenate(want[2]).astype(np.uint8).tolist()
    assert after[12] > 0 and np.array_equal(after[:12], before[:12])
    for bad in (-1, 17):
        rc, _, _, _, done = _c_call(gpu_ctx, bad)
        assert rc == sgpu.SGPU_EINVAL and (done == -7).all(), bad
    rc, om16, *_ = _c_call(gpu_ctx, 16)
    assert rc == sgpu.SGPU_OK and om16.tobytes() == _host("H", 16)[0].tobytes()
    # out_rounds = NULL, out_mask = NULL: the other outputs as before
    rc, om, oi, ok, done = _c_call(gpu_ctx, 3, out_rounds=False, mask=False)
    assert rc == sgpu.SGPU_OK and om.tobytes() == want[0].tobytes() and oi.tolist() == want[1].tolist()
    assert (done == -7).all() and not ok.any()
    # rounds = 0 fills out_rounds with zeros
    rc, om, oi, _, done = _c_call(gpu_ctx, 0)
    assert rc == sgpu.SGPU_OK and not done.any() and om.tobytes() == _host("H", 0)[0].tobytes()
    with pytest.raises(RuntimeError):
        loc, off, pairs, matches, _ = G.pair_list("H")
        gpu_ctx.estimate_batch_refined(loc, off, pairs, matches, rounds=17)


def test_binding_rejects_wrong_shapes():
    """The binding's ValueErrors come before any C call: no device, no library needed."""
    ctx = sgpu.SiftContext.__new__(sgpu.SiftContext)
    ctx._ctx = None
    loc = np.zeros((10, 2), np.float32)
    m = np.zeros((3, 2), np.int32)
    with pytest.raises(ValueError):
        ctx.estimate_batch_refined(np.zeros((10, 4), np.float32), [0, 4, 10], [(0, 1)], [m])
    with pytest.raises(ValueError):
        ctx.estimate_batch_refined(loc, [0, 4, 11], [(0, 1)], [m])
    with pytest.raises(ValueError):
        ctx.estimate_batch_refined(loc, [0, 4, 10], [(0, 1)], [m], model="E")
    with pytest.raises(ValueError):
        ctx.estimate_images_refined([(0, 1), (1, 0)], [m])


# ---- 5: extract -> match -> refined estimate -> guided match -----------------------------------------

ROLLS = [(0, 0), (7, 11), (3, -5), (20, 2)]   # (rows, columns) each view is rolled by
IMAGE_PAIRS = [(0, 1), (1, 2), (2, 3), (0, 3), (3, 0)]


def _views():
    img = synth_image(320, 240, 55)
    return np.stack([np.roll(img, s, axis=(0, 1)) for s in ROLLS])


def _check_chain(gpu_ctx):
    thr = 2.0
    plain = gpu_ctx.match_images(IMAGE_PAIRS)
    assert min(len(m) for m in plain) > 50
    _, inliers0, _ = gpu_ctx.estimate_images(IMAGE_PAIRS, plain, "H", thr, 512, 9)
    refined = gpu_ctx.estimate_images_refined(IMAGE_PAIRS, plain, "H", thr, 512, 9, rounds=3)
    models, inliers, masks, done = refined
    # the same call on the downloaded x, y: byte for byte, and the host's result
    keys = [np.ascontiguousarray(gpu_ctx.features(i, descriptors=False)[0][:, :2], np.float32)
            for i in range(4)]
    off = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)
    loc = np.concatenate(keys)
    batch = gpu_ctx.estimate_batch_refined(loc, off, IMAGE_PAIRS, plain, "H", thr, 512, 9, rounds=3)
    _same(refined, batch)
    _same(batch, R.host_refine(loc, off, IMAGE_PAIRS, plain, "H", thr, 512, 9, rounds=3))
    assert (inliers >= inliers0).all() and (done <= 3).all()
    guided = gpu_ctx.match_images_guided(IMAGE_PAIRS, H=models, hdistmax=thr)
    for p, (a, b) in enumerate(IMAGE_PAIRS):
        assert inliers[p] == masks[p].sum() and inliers[p] > 0.5 * len(plain[p]), (p, inliers[p])
        # the guided pass under the refined model keeps every refined inlier
        kept = set(map(tuple, guided[p].tolist()))
        assert set(map(tuple, plain[p][masks[p]].tolist())) <= kept, p


@gpu
def test_extract_match_refine_guided_chain(gpu_ctx):
    gpu_ctx.set_options(default_options())
    views = _views()
    gpu_ctx.extract(views)
    _check_chain(gpu_ctx)
    try:
        gpu_ctx.set_debug_flags(gpu_ctx.DEBUG_PARTS2)
        gpu_ctx.extract(views)
        _check_chain(gpu_ctx)
    finally:
        gpu_ctx.set_debug_flags(0)
