"""sgpu_estimate_batch / sgpu_estimate_images: one H or F per matched pair, on the device.

Expected values never come from the library: they are sgeo::estimate_host's (csrc/sift_geom.h),
run by the stand-alone program tests/abi/geom_check.cpp, built plain with g++ at test time.  The
device's models (as bytes), inlier counts and masks must be bit-identical to it; a mismatch is a
finding in the operation order, there is no tolerance.  What estimate_host computes is pinned on the
CPU by test_geom.py against the oracle's guided test and the planted scenes.

Hypothesis t of a pair draws by a hash of (seed, pair position, t, draw): a pair's result depends
on its position in the list, so the launch-independence test compares the real pairs among 3,000
fillers with the host's result for that same list, and holds them to the planted-recovery
condition of test 1."""
import functools

import numpy as np
import pytest

import geom_scenes as G
import sgpu
from sgpu_types import default_options
from sift_synth import synth_image

gpu = pytest.mark.gpu


def _same(got, want):
    gm, gi, gk = got
    wm, wi, wk = want
    assert gm.shape == wm.shape and gm.dtype == wm.dtype == np.float32
    bad = [p for p in range(len(wm)) if gm[p].tobytes() != wm[p].tobytes()]
    assert not bad, (bad[:8], gm[bad[0]], wm[bad[0]])
    assert gi.tolist() == wi.tolist()
    assert len(gk) == len(wk)
    for p, (a, b) in enumerate(zip(gk, wk)):
        assert a.dtype == bool and np.array_equal(a, b), p


def _recovered(masks, p, planted):
    return int((masks[p] & planted).sum()) >= 0.95 * int(planted.sum())


@functools.lru_cache(maxsize=None)
def _host(model):
    case = G.H_CASE if model == "H" else G.F_CASE
    loc, off, pairs, matches, _ = G.pair_list(model)
    return G.host_estimate(loc, off, pairs, matches, **case)


# ---- 1: the planted scenes and the edge pairs -----------------------------------------------------

@gpu
@pytest.mark.parametrize("model", ["H", "F"])
def test_planted_scenes_and_edge_pairs(gpu_ctx, model):
    """geom_scenes.pair_list: the scene, an empty pair between real ones, (b, a), the repeat,
    m = 0, S - 1, S, S + 1, a pair at one point, an empty set; set 0 starts at buffer row 5."""
    case = G.H_CASE if model == "H" else G.F_CASE
    loc, off, pairs, matches, planted = G.pair_list(model)
    assert off[0] == 5
    want = _host(model)
    assert _recovered(want[2], 0, planted) and _recovered(want[2], 3, planted)
    assert not want[0][8].any() and not want[0][5].any() and want[1][6] == G.MIN_SAMPLE[model]
    got = gpu_ctx.estimate_batch(loc, off, pairs, matches, **case)
    _same(got, want)


@gpu
def test_device_resident_locations(gpu_ctx):
    """SGPU_INPUT_DEVICE: the locations are read in place, 8 bytes into an allocation."""
    import devmem
    loc, off, pairs, matches, _ = G.pair_list("H")
    with devmem.uploaded(loc, offset=8) as addr:
        got = gpu_ctx.estimate_batch(None, off, pairs, matches, device_ptr=addr, **G.H_CASE)
    _same(got, _host("H"))


# ---- 2: hypothesis block edges, the lowest t among equal counts ----------------------------------

@functools.lru_cache(maxsize=None)
def _grid_scene():
    """40 matches of an exact integer translation on a coarse grid: every valid sample solves to
    the translation and counts all 40, many samples are collinear (invalid), so the winner is
    decided by t alone."""
    rng = np.random.Generator(np.random.PCG64(5))
    cells = rng.permutation(8 * 6)[:40]
    la = np.stack([40.0 + 60 * (cells % 8), 30.0 + 70 * (cells // 8)], 1).astype(np.float32)
    lb = la + np.array([7.0, -3.0], np.float32)
    m = np.stack([np.arange(40)] * 2, 1).astype(np.int32)
    return np.concatenate([la, lb]), np.array([0, 40, 80], np.int64), m


@gpu
@pytest.mark.parametrize("iterations", [1, 63, 64, 65, 256, 257])
def test_hypothesis_block_edges(gpu_ctx, iterations):
    for model in ("H", "F"):
        case = dict(G.H_CASE if model == "H" else G.F_CASE, iterations=iterations)
        loc, off, pairs, matches, _ = G.pair_list(model)
        want = G.host_estimate(loc, off, pairs[:4], matches[:4], **case)
        _same(gpu_ctx.estimate_batch(loc, off, pairs[:4], matches[:4], **case), want)
    loc, off, m = _grid_scene()
    pairs, ms = [(0, 1)] * 6, [m] * 6
    want = G.host_estimate(loc, off, pairs, ms, "H", 0.5, iterations, 3)
    if iterations >= 63:
        # every pair position found a valid sample, and every one of them counts all 40
        assert want[1].tolist() == [40] * 6
    for p in range(6):
        if want[1][p]:
            M = want[0][p].astype(np.float64) / float(want[0][p][2, 2])
            assert np.allclose(M, [[1, 0, 7], [0, 1, -3], [0, 0, 1]], atol=1e-4)
    _same(gpu_ctx.estimate_batch(loc, off, pairs, ms, "H", 0.5, iterations, 3), want)


def test_grid_scene_winner_is_the_lowest_valid_t():
    """The host reference on the grid scene, checked without a device: with every valid hypothesis
    at the same count, one more hypothesis never changes a winner once there is one (the lowest t
    wins), and the first hypotheses of some pair position are invalid (collinear)."""
    loc, off, m = _grid_scene()
    pairs, ms = [(0, 1)] * 6, [m] * 6
    prev, seen_invalid_first = None, False
    for it in (1, 2, 3, 4, 8, 64):
        models, inliers, _ = G.host_estimate(loc, off, pairs, ms, "H", 0.5, it, 3)
        if prev is not None:
            for p in range(6):
                if prev[1][p]:
                    assert inliers[p] == 40 and models[p].tobytes() == prev[0][p].tobytes()
                elif inliers[p]:
                    seen_invalid_first = True
        prev = (models, inliers)
    assert prev[1].tolist() == [40] * 6 and seen_invalid_first


# ---- 3: match tile edges ---------------------------------------------------------------------------

@gpu
def test_match_tile_edges(gpu_ctx):
    tile = G.header_constants()["tile"]
    assert tile >= 64
    for m in (tile - 1, tile, tile + 1, 2 * tile + 1):
        la, lb, mt, planted = G.h_scene(seed=300 + (m % 7), n=m, n_planted=(3 * m) // 5)
        loc = np.concatenate([la, lb])
        off = np.array([0, m, 2 * m], np.int64)
        want = G.host_estimate(loc, off, [(0, 1)], [mt], **G.H_CASE)
        assert _recovered(want[2], 0, planted)
        _same(gpu_ctx.estimate_batch(loc, off, [(0, 1)], [mt], **G.H_CASE), want)
    la, lb, mt, planted = G.f_scene(seed=310, n=tile + 1, n_planted=(7 * (tile + 1)) // 10)
    loc = np.concatenate([la, lb])
    off = np.array([0, tile + 1, 2 * tile + 2], np.int64)
    want = G.host_estimate(loc, off, [(0, 1)], [mt], **G.F_CASE)
    assert _recovered(want[2], 0, planted)
    _same(gpu_ctx.estimate_batch(loc, off, [(0, 1)], [mt], **G.F_CASE), want)


# ---- 4: launch independence ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _filler_list():
    """3,000 filler pairs of m = 4 (the first four planted matches) with the scene at positions
    0, 1023, 1024, 1025 and last."""
    loc, off, pairs, matches, planted = G.pair_list("H")
    fill = matches[0][planted][:4]
    real = [0, 1023, 1024, 1025, 3004]
    ps = [(0, 1)] * 3005
    ms = [matches[0] if p in real else fill for p in range(3005)]
    return loc, off, ps, ms, planted, real


@gpu
def test_launch_independence(gpu_ctx):
    loc, off, ps, ms, planted, real = _filler_list()
    want = G.host_estimate(loc, off, ps, ms, **G.H_CASE)
    for p in real:
        assert _recovered(want[2], p, planted)
    assert want[1][1] == 4 and want[1][2000] == 4
    got = gpu_ctx.estimate_batch(loc, off, ps, ms, **G.H_CASE)
    _same(got, want)
    # position 0 is test 1's position 0: the same result, whatever follows it in the list
    first = _host("H")
    assert got[0][0].tobytes() == first[0][0].tobytes() and np.array_equal(got[2][0], first[2][0])
    before = gpu_ctx.alloc_count()
    _same(gpu_ctx.estimate_batch(loc, off, ps, ms, **G.H_CASE), want)
    assert gpu_ctx.alloc_count() == before


# ---- 5: determinism and seeding --------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("model", ["H", "F"])
def test_determinism_and_seeding(gpu_ctx, model):
    case = G.H_CASE if model == "H" else G.F_CASE
    loc, off, pairs, matches, planted = G.pair_list(model)
    a = gpu_ctx.estimate_batch(loc, off, pairs, matches, **case)
    b = gpu_ctx.estimate_batch(loc, off, pairs, matches, **case)
    _same(a, b)
    other = dict(case, seed=case["seed"] + 1000)
    c = gpu_ctx.estimate_batch(loc, off, pairs, matches, **other)
    assert c[0][0].tobytes() != a[0][0].tobytes()
    assert _recovered(c[2], 0, planted) and _recovered(c[2], 3, planted)
    _same(c, G.host_estimate(loc, off, pairs, matches, **other))


# ---- 6: extract -> match -> estimate -> guided match ------------------------------------------------

ROLLS = [(0, 0), (7, 11), (3, -5), (20, 2)]   # (rows, columns) each view is rolled by
IMAGE_PAIRS = [(0, 1), (1, 2), (2, 3), (0, 3), (3, 0)]


def _views():
    img = synth_image(320, 240, 55)
    return np.stack([np.roll(img, s, axis=(0, 1)) for s in ROLLS])


def _check_chain(gpu_ctx):
    thr = 2.0
    plain = gpu_ctx.match_images(IMAGE_PAIRS)
    assert min(len(m) for m in plain) > 50
    models, inliers, masks = gpu_ctx.estimate_images(IMAGE_PAIRS, plain, "H", thr, 512, 9)
    # the same call on the downloaded x, y: byte for byte, and the host's result
    keys = [np.ascontiguousarray(gpu_ctx.features(i, descriptors=False)[0][:, :2], np.float32)
            for i in range(4)]
    off = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)
    loc = np.concatenate(keys)
    batch = gpu_ctx.estimate_batch(loc, off, IMAGE_PAIRS, plain, "H", thr, 512, 9)
    _same((models, inliers, masks), batch)
    _same(batch, G.host_estimate(loc, off, IMAGE_PAIRS, plain, "H", thr, 512, 9))
    guided = gpu_ctx.match_images_guided(IMAGE_PAIRS, H=models, hdistmax=thr)
    for p, (a, b) in enumerate(IMAGE_PAIRS):
        assert inliers[p] == masks[p].sum() and inliers[p] > 0.5 * len(plain[p]), (p, inliers[p])
        # the model maps the inliers within the threshold of the roll's translation
        d = np.array([ROLLS[b][1] - ROLLS[a][1], ROLLS[b][0] - ROLLS[a][0]], np.float64)
        x1 = keys[a][plain[p][masks[p], 0]].astype(np.float64)
        h = np.c_[x1, np.ones(len(x1))] @ models[p].astype(np.float64).T
        assert np.abs(h[:, :2] / h[:, 2:] - (x1 + d)).max() < thr, p
        # the guided pass under the model keeps every putative match that was an inlier
        kept = set(map(tuple, guided[p].tolist()))
        assert set(map(tuple, plain[p][masks[p]].tolist())) <= kept, p


@gpu
def test_extract_match_estimate_guided_chain(gpu_ctx):
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


# ---- 7: errors and states --------------------------------------------------------------------------

def _c_call(gpu_ctx, loc, off, nsets, pairs, matches, counts, model=0, threshold=2.0, iterations=16,
            seed=1, models=True, inliers=True):
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    mt = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
    ct = np.ascontiguousarray(counts, np.int32)
    lc = np.ascontiguousarray(loc, np.float32)
    of = np.ascontiguousarray(off, np.int64)
    om = np.zeros((max(len(pr), 1), 9), np.float32)
    oi = np.zeros(max(len(pr), 1), np.int32)
    ok = np.zeros(max(len(mt), 1), np.uint8)
    return sgpu.lib().sgpu_estimate_batch(
        gpu_ctx._ctx, lc.ctypes.data, of.ctypes.data, nsets, pr.ctypes.data, len(pr),
        mt.ctypes.data, ct.ctypes.data, model, threshold, iterations, seed,
        om.ctypes.data if models else None, oi.ctypes.data if inliers else None, ok.ctypes.data,
        sgpu.SGPU_INPUT_HOST)


def _times(gpu_ctx, n=13):
    t = np.full(n, -1.0, np.float32)
    assert sgpu.lib().sgpu_last_timing(gpu_ctx._ctx, t.ctypes.data, n) == sgpu.SGPU_OK
    return t


@gpu
def test_bad_arguments(gpu_ctx):
    loc, off, m = _grid_scene()
    good = dict(loc=loc, off=off, nsets=2, pairs=[(0, 1)], matches=m, counts=[40])
    assert _c_call(gpu_ctx, **good) == sgpu.SGPU_OK
    bad = [dict(pairs=[(0, 2)]), dict(pairs=[(-1, 1)]), dict(off=[0, 40, 39]), dict(counts=[-1]),
           dict(matches=np.r_[m[:39], [[40, 0]]]), dict(matches=np.r_[m[:39], [[0, 40]]]),
           dict(matches=np.r_[m[:39], [[-1, 0]]]), dict(iterations=0), dict(iterations=65537),
           dict(model=2), dict(model=-1), dict(models=False), dict(inliers=False)]
    for b in bad:
        assert _c_call(gpu_ctx, **dict(good, **b)) == sgpu.SGPU_EINVAL, b
    assert _c_call(gpu_ctx, **dict(good, iterations=65536, counts=[3], matches=m[:3])) == sgpu.SGPU_OK
    with pytest.raises(RuntimeError):
        gpu_ctx.estimate_batch(loc, off, [(0, 1)], [np.r_[m[:5], [[3, 40]]]])
    with pytest.raises(ValueError):
        gpu_ctx.estimate_batch(loc, off, [(0, 1)], [m], model="E")
    with pytest.raises(ValueError):
        gpu_ctx.estimate_batch(loc, off, [(0, 1)], [m, m])
    models, inliers, masks = gpu_ctx.estimate_batch(loc, off, [], [])
    assert models.shape == (0, 3, 3) and len(inliers) == 0 and masks == []


@gpu
def test_states_and_timing(gpu_ctx):
    views = _views()
    gpu_ctx.set_options(default_options())
    gpu_ctx.extract(views)
    plain = gpu_ctx.match_images(IMAGE_PAIRS[:2])
    before = _times(gpu_ctx)
    models, inliers, _ = gpu_ctx.estimate_images(IMAGE_PAIRS[:2], plain, "F", 4.0, 64, 2)
    after = _times(gpu_ctx)
    assert after[12] > 0 and np.array_equal(after[:12], before[:12])
    assert len(gpu_ctx.timing()) == 10
    assert (inliers >= 8).all()
    with pytest.raises(RuntimeError):
        gpu_ctx.estimate_images([(0, 4)], plain[:1])
    with pytest.raises(RuntimeError):   # a match index outside image 3's features
        gpu_ctx.estimate_images([(0, 3)], [np.array([[0, gpu_ctx.count(3)]], np.int32)])
    gpu_ctx.extract_stream([views[:2], views[2:]], cap=20000)
    with pytest.raises(RuntimeError):   # no last batch
        gpu_ctx.estimate_images(IMAGE_PAIRS[:2], plain)
    gpu_ctx.extract(views)
    again, _, _ = gpu_ctx.estimate_images(IMAGE_PAIRS[:2], plain, "F", 4.0, 64, 2)
    assert again.tobytes() == models.tobytes()


def test_binding_rejects_wrong_shapes():
    """The binding's ValueErrors come before any C call: no device, no library needed."""
    ctx = sgpu.SiftContext.__new__(sgpu.SiftContext)
    ctx._ctx = None
    loc = np.zeros((10, 2), np.float32)
    m = np.zeros((3, 2), np.int32)
    with pytest.raises(ValueError):
        ctx.estimate_batch(np.zeros((10, 4), np.float32), [0, 4, 10], [(0, 1)], [m])
    with pytest.raises(ValueError):
        ctx.estimate_batch(loc, [0, 4, 11], [(0, 1)], [m])
    with pytest.raises(ValueError):
        ctx.estimate_batch(loc, [0, 4, 10], [(0, 1)], [m], model="E")
    with pytest.raises(ValueError):
        ctx.estimate_images([(0, 1), (1, 0)], [m])
