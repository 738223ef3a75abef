"""sgpu_verify_batch / sgpu_verify_images: putative matching, refined H and / or F estimation and
guided matching of a whole pair list in one call, nothing crossing PCIe in between.

The contract is "the bits of the chain", so every expected value is the chain itself, run through
the separate bindings on the same context: match_batch -> estimate_batch_refined (per model) ->
match_batch_guided (the *_images forms after an extract).  Those are pinned by their own tests
against the CPU oracle and sgeo::estimate_host / refine_host.  Every comparison is equality of
bytes; there is no tolerance.  The synthetic pair list is built so that the chain's putative counts
hit 0, S - 1, S and S + 1 of both models (checked with the CPU oracle's matcher when the list is
built, and asserted on the chain's counts), which is where the fused call's estimator items differ
from the separate call's: it has items for pairs below the minimal sample."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_py as O
import sgpu
from sgpu_types import default_options
from sift_synth import quantize, synth_descriptors, synth_image

gpu = pytest.mark.gpu

# sgpu_default_verify_params, as the header documents them
DEFAULTS = dict(distmax=0.7, ratiomax=0.8, mutual_best_match=1, max_match=4096, h_threshold=2.0,
                f_threshold=4.0, hdistmax=2.0, fdistmax=4.0, iterations=512, seed=0, refine_rounds=3)
MODES = [(True, False), (False, True), (True, True)]


def _params(kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _chain(match, estimate, guided, H, F, cap, kw):
    """The three (or four) separate calls: match() -> the putative list, estimate(P, model, ...) per
    requested model, guided(Hm, Fm, cap) -> the verified list.  Returns verify_*'s tuple."""
    p = _params(kw)
    P = match(distmax=p["distmax"], ratiomax=p["ratiomax"], mbm=p["mutual_best_match"],
              max_match=p["max_match"])
    res = {}
    for name, want in (("H", H), ("F", F)):
        if want:
            m, i, _, _ = estimate(P, name, p["h_threshold" if name == "H" else "f_threshold"],
                                  p["iterations"], p["seed"], rounds=p["refine_rounds"])
            res[name] = (m, i)
    Hm, iH = res.get("H", (None, None))
    Fm, iF = res.get("F", (None, None))
    G = guided(Hm, Fm, distmax=p["distmax"], ratiomax=p["ratiomax"], hdistmax=p["hdistmax"],
               fdistmax=p["fdistmax"], mbm=p["mutual_best_match"], max_match=p["max_match"], cap=cap)
    return G, Hm, iH, Fm, iF, np.array([len(m) for m in P], np.int32), P


def _chain_batch(ctx, buf, loc, off, pairs, H=True, F=False, cap=None, **kw):
    return _chain(lambda **a: ctx.match_batch(buf, off, pairs, **a),
                  lambda P, *a, **k: ctx.estimate_batch_refined(loc, off, pairs, P, *a, **k),
                  lambda Hm, Fm, **a: ctx.match_batch_guided(buf, loc, off, pairs, Hm, Fm, **a),
                  H, F, cap, kw)


def _chain_images(ctx, pairs, H=True, F=False, cap=None, **kw):
    return _chain(lambda **a: ctx.match_images(pairs, **a),
                  lambda P, *a, **k: ctx.estimate_images_refined(pairs, P, *a, **k),
                  lambda Hm, Fm, **a: ctx.match_images_guided(pairs, Hm, Fm, **a),
                  H, F, cap, kw)


def _same(got, want):
    """verify_*'s tuple against the chain's: matches, models (bytes), inliers, putative counts."""
    gm, gH, giH, gF, giF, gp = got
    wm, wH, wiH, wF, wiF, wp = want[:6]
    assert gp.dtype == np.int32 and gp.tolist() == wp.tolist()
    for g, w, gi, wi, name in ((gH, wH, giH, wiH, "H"), (gF, wF, giF, wiF, "F")):
        if w is None:
            assert g is None and gi is None, name
            continue
        assert g.shape == w.shape and g.dtype == w.dtype == np.float32, name
        bad = [p for p in range(len(w)) if g[p].tobytes() != w[p].tobytes()]
        assert not bad, (name, bad[:8], g[bad[0]], w[bad[0]])
        assert gi.dtype == np.int32 and gi.tolist() == wi.tolist(), name
    assert len(gm) == len(wm)
    for p, (a, b) in enumerate(zip(gm, wm)):
        assert a.shape == b.shape and np.array_equal(a, b), (p, a.shape, b.shape)


# ---- 1: extract, then verify_images: the rolled views ---------------------------------------------

ROLLS = [(0, 0), (7, 11), (3, -5), (20, 2)]   # (rows, columns) each view is rolled by
IMAGE_PAIRS = [(0, 1), (1, 2), (2, 3), (0, 3), (3, 0)]


def _views():
    img = synth_image(320, 240, 55)
    return np.stack([np.roll(img, s, axis=(0, 1)) for s in ROLLS])


def _check_images(gpu_ctx):
    for rounds in (0, 3):
        for H, F in MODES:
            kw = dict(seed=9, refine_rounds=rounds)
            want = _chain_images(gpu_ctx, IMAGE_PAIRS, H, F, **kw)
            got = gpu_ctx.verify_images(IMAGE_PAIRS, H, F, **kw)
            _same(got, want)
            assert want[5].min() > 50
            if H and not F:
                assert min(len(m) for m in want[0]) > 25
                # hdistmax == h_threshold: the guided pass keeps every refined inlier of the
                # putative list (the masks come from the separate estimator call)
                P = want[6]
                _, _, masks, _ = gpu_ctx.estimate_images_refined(IMAGE_PAIRS, P, "H", 2.0, 512, 9,
                                                                 rounds=rounds)
                for p in range(len(IMAGE_PAIRS)):
                    assert got[2][p] == masks[p].sum() > 0.5 * len(P[p]), p
                    kept = set(map(tuple, got[0][p].tolist()))
                    assert set(map(tuple, P[p][masks[p]].tolist())) <= kept, p


@gpu
@pytest.mark.parametrize("parts2", [False, True])
def test_rolled_views(gpu_ctx, parts2):
    gpu_ctx.set_options(default_options())
    try:
        if parts2:
            gpu_ctx.set_debug_flags(gpu_ctx.DEBUG_PARTS2)
        gpu_ctx.extract(_views())
        _check_images(gpu_ctx)
    finally:
        gpu_ctx.set_debug_flags(0)


# ---- 2: verify_batch on synthetic sets --------------------------------------------------------------

A_ROWS = 300
# set index -> (rows, copies of set A's rows): the copies sit where a second pinhole view sees the
# row's point, the other rows are random descriptors at random places
COPY_SETS = {1: (127, 3), 2: (128, 4), 3: (129, 5), 5: (127, 7), 6: (128, 8), 7: (129, 9),
             8: (300, 90)}
A, EMPTY, BIG, ONE = 0, 4, 8, 9
# every small set against A (putative 3, 4, 5, 7, 8, 9); the scene, (b, a) beside it, (a, a), the
# repeat; two sets of copies of different rows (putative 0 with work to do); the one-row set; the
# empty set between real pairs, on both sides and alone
PAIRS = [(A, 1), (A, 2), (A, 3), (A, 5), (A, 6), (A, 7), (A, BIG), (BIG, A), (A, A), (A, BIG),
         (1, 5), (EMPTY, A), (A, 6), (A, EMPTY), (ONE, A), (A, ONE), (EMPTY, EMPTY), (2, A)]
WANT_PUTATIVE = {0: 3, 1: 4, 2: 5, 3: 7, 4: 8, 5: 9, 10: 0, 11: 0, 13: 0, 14: 1, 15: 1, 16: 0, 17: 4,
                 8: A_ROWS}


def _second_view(x1, depth):
    """Where the second of two pinhole views (f = 500, centre (320, 240)) sees the points."""
    K = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
    X = (np.c_[x1, np.ones(len(x1))] @ np.linalg.inv(K).T) * depth[:, None]
    ay, ax = 0.08, -0.03
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    c = (X @ (Ry @ Rx).T + np.array([0.6, 0.05, 0.1])) @ K.T
    return c[:, :2] / c[:, 2:]


@functools.lru_cache(maxsize=None)
def _synthetic():
    """(sets: list of (u8 descriptors, locations), buffer, locations, offsets).  Each copy set's
    seed is the first one for which the CPU oracle's matcher finds exactly the planted number of
    matches against A (and none between sets 1 and 5)."""
    rng = np.random.Generator(np.random.PCG64(4100))
    qa = quantize(synth_descriptors(A_ROWS, 4101))
    la = rng.uniform([0, 0], [640, 480], (A_ROWS, 2))
    seen = _second_view(la, rng.uniform(4, 8, A_ROWS))
    sets = {A: (qa, la.astype(np.float32)),
            EMPTY: (np.zeros((0, 128), np.uint8), np.zeros((0, 2), np.float32)),
            ONE: (qa[17:18].copy(), seen[17:18].astype(np.float32))}
    first = 0   # the copy sets take consecutive rows of A, so no two of the small ones share a row
    for s, (rows, copies) in COPY_SETS.items():
        src = np.arange(first, first + copies) if s != BIG else np.arange(A_ROWS - copies, A_ROWS)
        first += copies if s != BIG else 0
        for seed in range(4200 + 50 * s, 4250 + 50 * s):
            r = np.random.Generator(np.random.PCG64(seed))
            q = quantize(synth_descriptors(rows, seed))
            l = r.uniform([0, 0], [640, 480], (rows, 2))
            at = r.permutation(rows)[:copies]
            q[at] = qa[src]
            l[at] = seen[src] + r.uniform(-0.3, 0.3, (copies, 2))
            if s == BIG:
                l[at[::5]] += 150.0   # descriptor matches the geometry must reject
            ok = len(O.match(qa, q)) == copies
            if ok and s == 5:
                ok = len(O.match(sets[1][0], q)) == 0
            if ok:
                break
        else:
            raise AssertionError(f"no seed plants exactly {copies} matches in set {s}")
        sets[s] = (q, l.astype(np.float32))
    order = [sets[s] for s in range(10)]
    assert sorted({len(q) for q, _ in order}) == [0, 1, 127, 128, 129, 300]
    off = np.concatenate([[0], np.cumsum([len(q) for q, _ in order])]).astype(np.int64)
    buf = np.ascontiguousarray(np.concatenate([q for q, _ in order]), np.uint8)
    loc = np.ascontiguousarray(np.concatenate([l for _, l in order]), np.float32)
    return order, buf, loc, off


def _check_putative(counts):
    """The list exercises what it was built for: 0, S - 1, S, S + 1 of both models."""
    for p, c in WANT_PUTATIVE.items():
        assert counts[p] == c, (p, counts[p], c)
    assert {0, 3, 4, 5, 7, 8, 9} <= set(counts.tolist()) and counts[6] == 90 == counts[9]


_WANT = {}


def _want(gpu_ctx, H, F, **kw):
    """The chain's result on the synthetic list, computed once per parameter set and shared."""
    key = (H, F, tuple(sorted(kw.items())))
    if key not in _WANT:
        _, buf, loc, off = _synthetic()
        _WANT[key] = _chain_batch(gpu_ctx, buf, loc, off, PAIRS, H, F, **kw)
    return _WANT[key]


@gpu
@pytest.mark.parametrize("H,F", MODES)
def test_synthetic_sets_host_input(gpu_ctx, H, F):
    _, buf, loc, off = _synthetic()
    want = _want(gpu_ctx, H, F)
    _check_putative(want[5])
    # a pair below a model's minimal sample has no model and no verified match; at it, it has one
    for X, below in ((want[1], 0), (want[3], 3)):   # the pairs of 3 and of 7 putative matches
        if X is not None:
            assert not X[below].any() and len(want[0][below]) == 0
            assert not X[10].any() and not X[14].any() and not X[11].any()
    if H:
        assert want[1][1].any() and want[2][1] == 4 and want[2][8] == A_ROWS
    if F:
        assert want[4][6] >= 50 and 0 < len(want[0][6]) < 90 and want[4][4] == 8
    _same(gpu_ctx.verify_batch(buf, loc, off, PAIRS, H, F), want)


@gpu
def test_synthetic_sets_device_input(gpu_ctx):
    """SGPU_INPUT_DEVICE: descriptors and locations read in place (the locations 8 bytes into
    their allocation)."""
    import devmem
    _, buf, loc, off = _synthetic()
    with devmem.uploaded(buf) as d_addr, devmem.uploaded(loc, offset=8) as l_addr:
        got = gpu_ctx.verify_batch(None, None, off, PAIRS, True, True, device_ptrs=(d_addr, l_addr))
    _same(got, _want(gpu_ctx, True, True))


@gpu
def test_rounds_zero_and_not_mutual(gpu_ctx):
    _, buf, loc, off = _synthetic()
    for kw in (dict(refine_rounds=0), dict(mutual_best_match=0, iterations=300, seed=5)):
        want = _want(gpu_ctx, True, True, **kw)
        assert want[5].sum() > 500
        _same(gpu_ctx.verify_batch(buf, loc, off, PAIRS, True, True, **kw), want)


# ---- 3: max_match and cap ----------------------------------------------------------------------------

@gpu
def test_max_match_truncates_both_passes(gpu_ctx):
    """max_match below a pair's putative count: the estimator gets the same prefix as the chain's."""
    _, buf, loc, off = _synthetic()
    want = _want(gpu_ctx, True, True, max_match=10)
    assert want[5].tolist() == [min(c, 10) for c in _want(gpu_ctx, True, True)[5].tolist()]
    assert want[5][6] == 10 and want[5][8] == 10
    _same(gpu_ctx.verify_batch(buf, loc, off, PAIRS, True, True, max_match=10), want)


@gpu
def test_cap_below_the_verified_total(gpu_ctx):
    _, buf, loc, off = _synthetic()
    full = _want(gpu_ctx, True, False)
    counts = [len(m) for m in full[0]]
    k = 8   # the cap ends inside pair 8, (a, a)
    cap = sum(counts[:k]) + counts[k] // 2
    assert counts[k] >= 2 and sum(counts[k + 1:]) > 0 and sum(counts[:k]) > 0
    with pytest.raises(sgpu.MatchOverflow) as chain:
        _chain_batch(gpu_ctx, buf, loc, off, PAIRS, True, False, cap=cap)
    with pytest.raises(sgpu.MatchOverflow) as ei:
        gpu_ctx.verify_batch(buf, loc, off, PAIRS, True, False, cap=cap)
    assert ei.value.counts.tolist() == chain.value.counts.tolist() == counts
    assert len(ei.value.matches) == len(chain.value.matches) == k
    for a, b in zip(ei.value.matches, chain.value.matches):
        assert np.array_equal(a, b)
    # the models and the putative counts are complete all the same
    Hm, iH, Fm, iF, put = ei.value.verified
    assert Hm.tobytes() == full[1].tobytes() and iH.tolist() == full[2].tolist() and Fm is None
    assert put.tolist() == full[5].tolist()
    # the C call: SGPU_ERANGE, the leading pairs written, nothing behind them
    rc, out, cnt = _c_call(gpu_ctx, cap=cap)[:3]
    assert rc == sgpu.SGPU_ERANGE and cnt.tolist() == counts
    lead = sum(counts[:k])
    assert np.array_equal(out[:lead], np.concatenate(full[0][:k])) and (out[lead:] == -9).all()
    # a cap that holds exactly everything
    _same(gpu_ctx.verify_batch(buf, loc, off, PAIRS, True, False, cap=sum(counts)), full)


# ---- 4: launch independence, repeated shapes --------------------------------------------------------

@gpu
def test_launch_independence(gpu_ctx):
    """300 filler pairs of the one-row set with the scene at positions 0, 63, 64 and last: a pair's
    result depends on its position only through the sampler, exactly as in the chain; a second
    call of the same shape allocates nothing."""
    _, buf, loc, off = _synthetic()
    real = [0, 63, 64, 303]
    pairs = [(A, BIG) if p in real else (ONE, ONE) for p in range(304)]
    want = _chain_batch(gpu_ctx, buf, loc, off, pairs, True, True)
    assert all(want[5][p] == 90 and len(want[0][p]) > 0 for p in real)
    assert want[5].sum() == 4 * 90 + 300
    got = gpu_ctx.verify_batch(buf, loc, off, pairs, True, True)
    _same(got, want)
    # position 0 is the stand-alone call's position 0, whatever follows it
    alone = gpu_ctx.verify_batch(buf, loc, off, [(A, BIG)], True, True)
    assert alone[1][0].tobytes() == got[1][0].tobytes() and alone[3][0].tobytes() == got[3][0].tobytes()
    assert np.array_equal(alone[0][0], got[0][0])
    # ... and to the sizes of the list above again
    got = gpu_ctx.verify_batch(buf, loc, off, pairs, True, True)
    before = gpu_ctx.alloc_count()
    _same(gpu_ctx.verify_batch(buf, loc, off, pairs, True, True), want)
    assert gpu_ctx.alloc_count() == before


# ---- 5: determinism and timing -----------------------------------------------------------------------

def _times(gpu_ctx, n=14):
    t = np.full(n, -1.0, np.float32)
    assert sgpu.lib().sgpu_last_timing(gpu_ctx._ctx, t.ctypes.data, n) == sgpu.SGPU_OK
    return t


@gpu
def test_determinism_and_timing(gpu_ctx):
    _, buf, loc, off = _synthetic()
    _want(gpu_ctx, True, True)   # the separate calls have run: times[8], times[12] are theirs
    before = _times(gpu_ctx)
    assert before[8] > 0 and before[12] > 0
    a = gpu_ctx.verify_batch(buf, loc, off, PAIRS, True, True, seed=21)
    after = _times(gpu_ctx)
    assert after[13] > 0 and gpu_ctx.verify_time() == after[13]
    assert np.array_equal(after[:13], before[:13])
    assert list(gpu_ctx.timing()) == ["upload", "pyramid", "detect", "orientation", "expand",
                                      "descriptor", "download", "total", "match", "list"]
    b = gpu_ctx.verify_batch(buf, loc, off, PAIRS, True, True, seed=21)
    _same(a, b)
    c = gpu_ctx.verify_batch(buf, loc, off, PAIRS, True, True, seed=22)
    assert c[5].tolist() == a[5].tolist()
    assert c[1].tobytes() != a[1].tobytes() or c[3].tobytes() != a[3].tobytes()
    _same(c, _want(gpu_ctx, True, True, seed=22))


# ---- 6: errors -----------------------------------------------------------------------------------------

def _c_call(gpu_ctx, cap=4000, params="default", want_h=True, want_f=False, loc="host",
            desc="host", pairs=None, off=None, nsets=None, counts=True, out=True, **kw):
    """sgpu_verify_batch itself on the synthetic list: (return value, out [cap][2] prefilled
    with -9, counts prefilled with -7, H prefilled with 5)."""
    _, buf, lc, o = _synthetic()
    off = np.ascontiguousarray(o if off is None else off, np.int64)
    pr = np.ascontiguousarray(PAIRS if pairs is None else pairs, np.int32).reshape(-1, 2)
    vp = sgpu.SiftContext.verify_params(**kw) if params == "default" else params
    om = np.full((max(cap, 1), 2), -9, np.int32)
    cnt = np.full(len(pr), -7, np.int32)
    H = np.full((len(pr), 9), 5.0, np.float32)
    F = np.full((len(pr), 9), 5.0, np.float32)
    rc = sgpu.lib().sgpu_verify_batch(
        gpu_ctx._ctx, buf.ctypes.data if desc == "host" else None,
        lc.ctypes.data if loc == "host" else None, off.ctypes.data,
        len(off) - 1 if nsets is None else nsets, pr.ctypes.data, len(pr),
        None if vp is None else ctypes.byref(vp), H.ctypes.data if want_h else None, None,
        F.ctypes.data if want_f else None, None, None, om.ctypes.data if out else None, cap,
        cnt.ctypes.data if counts else None, sgpu.SGPU_INPUT_HOST)
    return rc, om, cnt, H


@gpu
def test_bad_arguments(gpu_ctx):
    _, buf, loc, off = _synthetic()
    rc, _, cnt, H = _c_call(gpu_ctx)
    assert rc == sum(cnt) > 300 and (cnt >= 0).all() and not (H == 5.0).all()
    bad = [dict(params=None), dict(iterations=0), dict(iterations=65537), dict(refine_rounds=-1),
           dict(refine_rounds=17), dict(want_h=False, want_f=False), dict(loc=None),
           dict(desc=None), dict(pairs=[(0, 10)]), dict(pairs=[(-1, 0)]),
           dict(off=[0, 300, 200] + off[3:].tolist()), dict(nsets=-1), dict(counts=False),
           dict(out=False)]
    for kw in bad:
        rc, om, cnt, H = _c_call(gpu_ctx, **kw)
        # refused on the host: nothing was written
        assert rc == sgpu.SGPU_EINVAL, kw
        assert (om == -9).all() and (cnt == -7).all() and (H == 5.0).all(), kw
    # out_pairs may be NULL with cap 0; every pair index is checked, not only the first
    rc, _, cnt, _ = _c_call(gpu_ctx, cap=0, out=False, pairs=[(EMPTY, A), (A, EMPTY)])
    assert rc == 0 and cnt.tolist() == [0, 0]
    assert _c_call(gpu_ctx, pairs=PAIRS + [(0, 10)])[0] == sgpu.SGPU_EINVAL
    with pytest.raises(RuntimeError):
        gpu_ctx.verify_batch(buf, loc, off, [(0, 10)])
    with pytest.raises(RuntimeError):
        gpu_ctx.verify_batch(buf, loc, off, PAIRS, iterations=0)
    got = gpu_ctx.verify_batch(buf, loc, off, [], True, True)
    assert got[0] == [] and got[1].shape == (0, 3, 3) and got[5].shape == (0,)
    # the context still works
    _same(gpu_ctx.verify_batch(buf, loc, off, PAIRS, True, False), _want(gpu_ctx, True, False))


@gpu
def test_verify_images_error_states(gpu_ctx):
    views = _views()
    gpu_ctx.set_options(default_options())
    gpu_ctx.extract_stream([views[:2], views[2:]], cap=20000)
    gpu_ctx.batch = 4   # the binding forgets the batch too; ask the library itself
    with pytest.raises(RuntimeError):
        gpu_ctx.verify_images([(0, 1)])
    try:
        gpu_ctx.set_options(default_options(descriptors=0))
        gpu_ctx.extract(views)
        with pytest.raises(RuntimeError):
            gpu_ctx.verify_images([(0, 1)])
    finally:
        gpu_ctx.set_options(default_options())
    gpu_ctx.extract(views)
    for bad in (dict(pairs=[(0, 4)]), dict(pairs=[(0, 1)], iterations=70000),
                dict(pairs=[(0, 1)], refine_rounds=17)):
        with pytest.raises(RuntimeError):
            gpu_ctx.verify_images(bad.pop("pairs"), **bad)
    got = gpu_ctx.verify_images([(0, 1)], True, True)
    assert len(got[0][0]) > 25 and got[2][0] > 25 and got[5][0] > 50
