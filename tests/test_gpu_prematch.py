"""Preemptive matching on the device: sgpu_select_top_scale_*, sgpu_prematch_batch and
sgpu_prematch_images.

1  The selection kernel against NumPy (tests/select_cases.py: the cases the CPU test gives
   sgsel::select_host), from host and from device-resident scales, one call per `top` over all sets.
2  prematch_batch = the chain: the NumPy selection, match_batch on the host-gathered subsets with
   max_match = top, the matches mapped back through the selected indices -- and the CPU oracle's
   matcher on the same subsets.  Equality of every count and every match; there is no tolerance.
3  prematch_images after an extract of nine small images (three scenes, three rolled views each):
   the same chain from the downloaded keys and u8 descriptors, and the candidate pairs.
No expected value comes from the code under test."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_py as O
import select_cases as SC
import sgpu
from sgpu_types import default_options
from sift_synth import quantize, synth_descriptors, synth_image

gpu = pytest.mark.gpu


# ---- 1: the selection ---------------------------------------------------------------------------------

def _check_selection(got, sets, top, how):
    assert len(got) == len(sets)
    for s, ((label, scale), g) in enumerate(zip(sets, got)):
        want = SC.numpy_select(scale, top)
        assert g.dtype == np.int32 and np.array_equal(g, want), \
            f"set {s} ({label}), size {len(scale)}, top {top}, {how}: got {g[:12]}..., want {want[:12]}..."


@gpu
@pytest.mark.parametrize("top", SC.TOPS)
def test_selection_equals_numpy(gpu_ctx, top):
    import devmem
    sets = SC.sets_for(top)
    flat = np.concatenate([s for _, s in sets]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in sets])]).astype(np.int64)
    assert {len(s) for _, s in sets} >= set(SC.SIZES)
    _check_selection(gpu_ctx.select_top_scale(flat, off, top), sets, top, "host, stride 1")
    wide = SC.strided(flat, 4, 2)   # the layout of a key buffer: the scale is column 2 of 4
    _check_selection(gpu_ctx.select_top_scale(wide, off, top, stride=4), sets, top, "host, stride 4")
    with devmem.uploaded(flat, offset=4) as addr:
        _check_selection(gpu_ctx.select_top_scale(None, off, top, device_ptr=addr), sets, top,
                         "device, stride 1")
    with devmem.uploaded(wide) as addr:
        _check_selection(gpu_ctx.select_top_scale(None, off, top, stride=4, device_ptr=addr), sets,
                         top, "device, stride 4")
    # the result is a pure function of the input
    a = gpu_ctx.select_top_scale(flat, off, top)
    b = gpu_ctx.select_top_scale(flat, off, top)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@gpu
def test_selection_bad_arguments(gpu_ctx):
    L = sgpu.lib()
    sc = np.arange(10, dtype=np.float32)
    off = np.array([0, 4, 10], np.int64)

    def call(scale=sc, stride=1, off=off, nsets=2, top=3, index=True, sub=True):
        idx = np.full(16, -9, np.int32)
        so = np.full(len(off), -7, np.int64)
        o = np.ascontiguousarray(off, np.int64)
        rc = L.sgpu_select_top_scale_batch(gpu_ctx._ctx, None if scale is None else scale.ctypes.data,
                                           stride, o.ctypes.data, nsets, top,
                                           idx.ctypes.data if index else None,
                                           so.ctypes.data if sub else None, sgpu.SGPU_INPUT_HOST)
        return rc, idx, so

    rc, idx, so = call()
    assert rc == sgpu.SGPU_OK and so.tolist() == [0, 3, 6] and idx[:6].tolist() == [1, 2, 3, 3, 4, 5]
    assert (idx[6:] == -9).all()
    for kw in (dict(top=0), dict(top=-1), dict(stride=0), dict(scale=None), dict(index=False),
               dict(sub=False), dict(off=np.array([0, 5, 4])), dict(off=np.array([-1, 4, 10])),
               dict(nsets=-1)):
        rc, idx, so = call(**kw)
        assert rc == sgpu.SGPU_EINVAL, kw
        assert (idx == -9).all() and (so == -7).all(), kw
    # empty sets only: nothing is read, nothing is written but the offsets
    rc, idx, so = call(scale=None, off=np.array([0, 0, 0]))
    assert rc == sgpu.SGPU_OK and so.tolist() == [0, 0, 0] and (idx == -9).all()


# ---- 2: prematch_batch on synthetic sets -----------------------------------------------------------------

SIZES = [0, 1, 99, 100, 101, 300, 300]
EMPTY, ONE, A, B = 0, 1, 5, 6
TOP = 100
DUPS = 60          # rows of set B that are near-copies of rows of set A ...
DUPS_IN = 30       # ... of which these lie in both sets' top 100 by scale, the rest in neither
PLANTED = 0        # PAIRS[0] = (A, B)
PAIRS = [(A, B), (B, A), (A, A), (A, B), (EMPTY, A), (A, EMPTY), (ONE, A), (2, 3), (3, 4), (4, B),
         (2, A), (ONE, ONE), (EMPTY, EMPTY), (B, 4)]


def _big_scales(rng, n, inside, outside):
    """Scales of a 300-row set: the rows `inside` and 69 others get distinct values in (20, 30),
    three rows tie at 15.0 -- the 100th largest, so one of them is taken -- and everything else,
    the rows `outside` among it, lies in (1, 10)."""
    sc = rng.uniform(1, 10, n).astype(np.float32)
    free = np.setdiff1d(np.arange(n), np.concatenate([inside, outside]))
    free = rng.permutation(free)
    high = np.concatenate([inside, free[:99 - len(inside)]])
    sc[high] = (20 + 10 * rng.permutation(len(high)) / len(high)).astype(np.float32)
    sc[free[99 - len(inside):102 - len(inside)]] = 15.0
    return sc


@functools.lru_cache(maxsize=None)
def _synthetic():
    """(sets [(u8 descriptors, scales)], descriptor buffer, scale buffer, offsets)."""
    rng = np.random.Generator(np.random.PCG64(5100))
    dA = synth_descriptors(300, 5101)
    src = rng.permutation(300)[:DUPS]                     # the rows of A that B copies
    dB = synth_descriptors(300, 5102, base=dA[src], n_dup=DUPS)
    at = rng.permutation(300)                             # B's row k moves to row at[k]
    pB = np.empty_like(dB)
    pB[at] = dB
    sA = _big_scales(rng, 300, src[:DUPS_IN], src[DUPS_IN:])
    sB = _big_scales(rng, 300, at[:DUPS_IN], at[DUPS_IN:DUPS])
    sets = {A: (quantize(dA), sA), B: (quantize(pB), sB),
            EMPTY: (np.zeros((0, 128), np.uint8), np.zeros(0, np.float32)),
            ONE: (quantize(dA[src[:1]]), np.array([3.0], np.float32))}
    for s in (2, 3, 4):   # 99, 100, 101 rows: near-copies of A's first rows among random ones
        d = synth_descriptors(SIZES[s], 5110 + s, base=dA, n_dup=25)
        sc = rng.uniform(1, 30, SIZES[s]).astype(np.float32)
        sc[5:9] = sc[4]   # equal scales inside a small set
        sets[s] = (quantize(d), sc)
    order = [sets[s] for s in range(len(SIZES))]
    assert [len(q) for q, _ in order] == SIZES
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    buf = np.ascontiguousarray(np.concatenate([q for q, _ in order]), np.uint8)
    scale = np.ascontiguousarray(np.concatenate([s for _, s in order]), np.float32)
    return order, buf, scale, off


def _subsets(order, top):
    """The NumPy selection of every set and the host-gathered subsets as one buffer."""
    sel = [SC.numpy_select(sc, top) for _, sc in order]
    sub = np.ascontiguousarray(np.concatenate([q[i] for (q, _), i in zip(order, sel)]), np.uint8)
    soff = np.concatenate([[0], np.cumsum([len(i) for i in sel])]).astype(np.int64)
    return sel, sub, soff


def _chain(gpu_ctx, order, pairs, top, mbm, **kw):
    """The expected matches of a pair list: match_batch on the gathered subsets with max_match =
    top, mapped back through the selection."""
    sel, sub, soff = _subsets(order, top)
    res = gpu_ctx.match_batch(sub, soff, pairs, mbm=mbm, max_match=top, **kw)
    return [np.stack([sel[a][m[:, 0]], sel[b][m[:, 1]]], axis=1).astype(np.int32)
            for (a, b), m in zip(pairs, res)], sel


_WANT = {}


def _want(gpu_ctx, mbm, top=TOP):
    key = (mbm, top)
    if key not in _WANT:
        order = _synthetic()[0]
        want, sel = _chain(gpu_ctx, order, PAIRS, top, mbm)
        # the CPU oracle's matcher on the same subsets says the same
        for (a, b), w in zip(PAIRS, want):
            qa, qb = order[a][0][sel[a]], order[b][0][sel[b]]
            m = O.match(qa, qb, mbm=mbm, max_match=top) if len(qa) and len(qb) else np.zeros((0, 2), np.int32)
            assert np.array_equal(np.stack([sel[a][m[:, 0]], sel[b][m[:, 1]]], axis=1), w), (a, b)
        _WANT[key] = want
    return _WANT[key]


def _same(got, want):
    counts, matches = got
    assert counts.dtype == np.int32 and counts.tolist() == [len(w) for w in want]
    assert len(matches) == len(want)
    for p, (g, w) in enumerate(zip(matches, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (p, g[:5], w[:5])


@gpu
@pytest.mark.parametrize("mbm", [1, 0])
def test_prematch_batch_is_the_chain(gpu_ctx, mbm):
    order, buf, scale, off = _synthetic()
    want = _want(gpu_ctx, mbm)
    # the selection took effect: the planted pair loses the duplicates outside the top rows
    full = len(O.match(order[A][0], order[B][0], mbm=mbm))
    sub = len(want[PLANTED])
    assert full >= DUPS - 5 and DUPS_IN - 5 <= sub <= DUPS_IN + 5 and sub != full, (full, sub)
    sel = SC.numpy_select(order[A][1], TOP)
    assert not np.array_equal(sel, np.arange(200, 300)) and (order[A][1][sel] == 15.0).sum() == 1
    assert any(len(w) for w in want[7:11]) and len(want[6]) == 1
    for p in (4, 5, 12):
        assert len(want[p]) == 0
    assert all((np.diff(w[:, 0]) > 0).all() for w in want if len(w) > 1)   # ascending first index
    _same(gpu_ctx.prematch_batch(buf, scale, off, PAIRS, TOP, mbm=mbm), want)
    # counts only: the same counts, no matches
    counts, none = gpu_ctx.prematch_batch(buf, scale, off, PAIRS, TOP, mbm=mbm, matches=False)
    assert none is None and counts.tolist() == [len(w) for w in want]


@gpu
def test_prematch_batch_strided_and_device_input(gpu_ctx):
    import devmem
    order, buf, scale, off = _synthetic()
    want = _want(gpu_ctx, 1)
    wide = SC.strided(scale, 4, 2)
    _same(gpu_ctx.prematch_batch(buf, wide, off, PAIRS, TOP, stride=4), want)
    with devmem.uploaded(buf) as d_addr, devmem.uploaded(wide, offset=8) as s_addr:
        _same(gpu_ctx.prematch_batch(None, None, off, PAIRS, TOP, stride=4,
                                     device_ptrs=(d_addr, s_addr)), want)


@gpu
def test_all_pairs_mode(gpu_ctx):
    order, buf, scale, off = _synthetic()
    n = len(SIZES)
    every = [(a, b) for a in range(n) for b in range(a + 1, n)]
    want, _ = _chain(gpu_ctx, order, every, TOP, 1)
    assert sum(len(w) for w in want) > 30
    _same(gpu_ctx.prematch_batch(buf, scale, off, None, TOP), want)
    _same(gpu_ctx.prematch_batch(buf, scale, off, every, TOP), want)
    counts, _ = gpu_ctx.prematch_batch(buf, scale, off, None, TOP, matches=False)
    assert counts.tolist() == [len(w) for w in want]
    # npairs must be nsets (nsets - 1) / 2
    for npairs in (len(every) - 1, len(every) + 1, 0):
        rc, _, cnt = _c_call(gpu_ctx, pairs=None, npairs=npairs)
        assert rc == sgpu.SGPU_EINVAL and (cnt == -7).all(), npairs


@gpu
def test_top_above_every_set_is_match_batch(gpu_ctx):
    order, buf, scale, off = _synthetic()
    for mbm in (1, 0):
        want = gpu_ctx.match_batch(buf, off, PAIRS, mbm=mbm, max_match=6000)
        assert len(want[PLANTED]) >= DUPS - 5
        _same(gpu_ctx.prematch_batch(buf, scale, off, PAIRS, 6000, mbm=mbm), want)


def _c_call(gpu_ctx, cap=4000, pairs=PAIRS, npairs=None, top=TOP, stride=1, off=None, nsets=None,
            desc=True, scale=True, counts=True, out=True, mbm=1):
    """sgpu_prematch_batch itself on the synthetic sets: (return value, out [cap][2] prefilled
    with -9, counts prefilled with -7)."""
    _, buf, sc, o = _synthetic()
    off = np.ascontiguousarray(o if off is None else off, np.int64)
    pr = None if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    if npairs is None:
        npairs = len(pr)
    om = np.full((max(cap, 1), 2), -9, np.int32)
    cnt = np.full(max(npairs, len(PAIRS), 1), -7, np.int32)
    rc = sgpu.lib().sgpu_prematch_batch(
        gpu_ctx._ctx, buf.ctypes.data if desc else None, sc.ctypes.data if scale else None, stride,
        off.ctypes.data, len(off) - 1 if nsets is None else nsets,
        None if pr is None else pr.ctypes.data, npairs, top, 0.7, 0.8, mbm,
        cnt.ctypes.data if counts else None, om.ctypes.data if out else None, cap,
        sgpu.SGPU_INPUT_HOST)
    return rc, om, cnt


@gpu
def test_counts_only_and_cap(gpu_ctx):
    order, buf, scale, off = _synthetic()
    want = _want(gpu_ctx, 1)
    counts = [len(w) for w in want]
    total = sum(counts)
    # out_pairs NULL: counts only, whatever cap says; the return value is the total
    rc, om, cnt = _c_call(gpu_ctx, cap=12345, out=False)
    assert rc == total and cnt[:len(PAIRS)].tolist() == counts and (om == -9).all()
    rc, _, cnt = _c_call(gpu_ctx, cap=0, out=False)
    assert rc == total and cnt[:len(PAIRS)].tolist() == counts
    # a cap that holds exactly everything: nothing behind the matches is written
    rc, om, cnt = _c_call(gpu_ctx, cap=total + 7)
    assert rc == total and np.array_equal(om[:total], np.concatenate(want)) and (om[total:] == -9).all()
    # a cap that ends inside pair 2, (A, A): SGPU_ERANGE, complete counts, the leading pairs
    k = 2
    cap = sum(counts[:k]) + counts[k] // 2
    assert counts[k] == TOP and sum(counts[:k]) > 0 and sum(counts[k + 1:]) > 0
    rc, om, cnt = _c_call(gpu_ctx, cap=cap)
    lead = sum(counts[:k])
    assert rc == sgpu.SGPU_ERANGE and cnt[:len(PAIRS)].tolist() == counts
    assert np.array_equal(om[:lead], np.concatenate(want[:k])) and (om[lead:] == -9).all()
    with pytest.raises(sgpu.MatchOverflow) as ei:
        gpu_ctx.prematch_batch(buf, scale, off, PAIRS, TOP, cap=cap)
    assert ei.value.counts.tolist() == counts and len(ei.value.matches) == k
    assert all(np.array_equal(a, b) for a, b in zip(ei.value.matches, want))


@gpu
def test_prematch_bad_arguments(gpu_ctx):
    order, buf, scale, off = _synthetic()
    bad_off = off.copy()
    bad_off[3] = bad_off[2] - 1
    bad = [dict(top=0), dict(top=-3), dict(stride=0), dict(scale=False), dict(desc=False),
           dict(counts=False), dict(pairs=[(0, 7)]), dict(pairs=[(-1, 0)]),
           dict(pairs=PAIRS + [(0, 7)]), dict(off=bad_off), dict(nsets=-1), dict(npairs=-1),
           dict(pairs=None, npairs=20)]
    for kw in bad:
        rc, om, cnt = _c_call(gpu_ctx, **kw)
        assert rc == sgpu.SGPU_EINVAL, kw
        assert (om == -9).all() and (cnt == -7).all(), kw   # refused on the host: nothing written
    with pytest.raises(RuntimeError):
        gpu_ctx.prematch_batch(buf, scale, off, [(0, 7)])
    with pytest.raises(RuntimeError):
        gpu_ctx.prematch_batch(buf, scale, off, PAIRS, top=0)
    counts, matches = gpu_ctx.prematch_batch(buf, scale, off, [])
    assert counts.shape == (0,) and matches == []
    # pairs of empty sets alone need no descriptors
    rc, _, cnt = _c_call(gpu_ctx, pairs=[(EMPTY, EMPTY)], off=np.zeros(len(off), np.int64),
                         desc=False, scale=False)
    assert rc == 0 and cnt[0] == 0
    # the context still works
    _same(gpu_ctx.prematch_batch(buf, scale, off, PAIRS, TOP), _want(gpu_ctx, 1))


def _times(gpu_ctx, n=15):
    t = np.full(n, -1.0, np.float32)
    assert sgpu.lib().sgpu_last_timing(gpu_ctx._ctx, t.ctypes.data, n) == sgpu.SGPU_OK
    return t


@gpu
def test_allocations_and_timing(gpu_ctx):
    order, buf, scale, off = _synthetic()
    want = _want(gpu_ctx, 1)            # match_batch has run: times[8] is its own
    gpu_ctx.prematch_batch(buf, scale, off, PAIRS, TOP)
    before = gpu_ctx.alloc_count()
    _same(gpu_ctx.prematch_batch(buf, scale, off, PAIRS, TOP), want)
    assert gpu_ctx.alloc_count() == before
    gpu_ctx.match_batch(buf, off, PAIRS)
    t0 = _times(gpu_ctx)
    assert t0[8] > 0
    gpu_ctx.prematch_batch(buf, scale, off, PAIRS, TOP)
    t1 = _times(gpu_ctx)
    assert t1[14] > 0 and gpu_ctx.prematch_time() == t1[14]
    assert np.array_equal(t1[:14], t0[:14])
    assert list(gpu_ctx.timing()) == ["upload", "pyramid", "detect", "orientation", "expand",
                                      "descriptor", "download", "total", "match", "list"]


# ---- 3: prematch_images: three scenes, three rolled views each -------------------------------------------

SEEDS = [55, 56, 57]
ROLLS = [(0, 0), (7, 11), (3, -5)]   # (rows, columns) each view is rolled by
SAME_SCENE = [(a, b) for a in range(9) for b in range(a + 1, 9) if a // 3 == b // 3]
EVERY = [(a, b) for a in range(9) for b in range(a + 1, 9)]


def _views():
    return np.stack([np.roll(synth_image(320, 240, s), r, axis=(0, 1)) for s in SEEDS for r in ROLLS])


def _check_images(gpu_ctx):
    feats = [(gpu_ctx.features(i)[0], gpu_ctx.features_u8(i)) for i in range(9)]
    order = [(q, np.ascontiguousarray(k[:, 2])) for k, q in feats]
    assert min(len(q) for q, _ in order) > 300
    sel = [SC.numpy_select(sc, 100) for _, sc in order]
    # the fixture does what it is there for (CPU oracle: images 4, 5 and 8): a scale tie at the
    # cut, taken in part, and selections that are no contiguous run of the feature list
    tied = []
    for i, ((_, sc), s) in enumerate(zip(order, sel)):
        key = SC.order_key(sc)
        T = np.sort(key)[::-1][99]
        if 0 < (key[s] == T).sum() < (key == T).sum():
            tied.append(i)
        assert not (np.diff(s) == 1).all(), i
    assert tied == [4, 5, 8], tied
    got_sel = gpu_ctx.select_top_scale_images(100)
    assert len(got_sel) == 9 and all(np.array_equal(g, w) for g, w in zip(got_sel, sel))
    want, _ = _chain(gpu_ctx, order, EVERY, 100, 1)
    for (a, b), w in zip(EVERY, want):
        m = O.match(order[a][0][sel[a]], order[b][0][sel[b]], max_match=100)
        assert np.array_equal(np.stack([sel[a][m[:, 0]], sel[b][m[:, 1]]], axis=1), w), (a, b)
    counts = np.array([len(w) for w in want])
    same = np.array([p in SAME_SCENE for p in EVERY])
    assert counts[same].min() >= 75 and counts[same].max() <= 88 and counts[~same].max() <= 2, counts
    _same(gpu_ctx.prematch_images(None, 100), want)
    _same(gpu_ctx.prematch_images(EVERY, 100), want)
    c, none = gpu_ctx.prematch_images(None, 100, matches=False)
    assert none is None and c.tolist() == counts.tolist()
    pairs, pc = gpu_ctx.candidate_pairs(top=100, min_matches=4)
    assert pairs.dtype == np.int32 and pairs.tolist() == [list(p) for p in SAME_SCENE]
    assert pc.tolist() == counts[same].tolist()
    # an explicit list with both orders, (a, a) and a repeat; top above every image
    some = [(3, 4), (4, 3), (5, 5), (3, 4), (0, 8)]
    _same(gpu_ctx.prematch_images(some, 100), _chain(gpu_ctx, order, some, 100, 1)[0])
    full = gpu_ctx.match_images(some, max_match=6000)
    _same(gpu_ctx.prematch_images(some, 6000), full)
    assert gpu_ctx.prematch_time() > 0


@gpu
@pytest.mark.parametrize("parts2", [False, True])
def test_prematch_images(gpu_ctx, parts2):
    gpu_ctx.set_options(default_options())
    try:
        if parts2:
            gpu_ctx.set_debug_flags(gpu_ctx.DEBUG_PARTS2)
        gpu_ctx.extract(_views())
        _check_images(gpu_ctx)
    finally:
        gpu_ctx.set_debug_flags(0)


@gpu
def test_prematch_images_error_states(gpu_ctx):
    views = _views()
    gpu_ctx.set_options(default_options())
    gpu_ctx.extract_stream([views[:3], views[3:6]], cap=20000)
    gpu_ctx.batch = 6   # the binding forgets the batch too; ask the library itself
    for call in (lambda: gpu_ctx.prematch_images([(0, 1)]), lambda: gpu_ctx.select_top_scale_images(100),
                 lambda: gpu_ctx.match_images([(0, 1)])):
        with pytest.raises(RuntimeError):
            call()
    try:
        gpu_ctx.set_options(default_options(descriptors=0))
        gpu_ctx.extract(views[:3])
        for call in (lambda: gpu_ctx.prematch_images([(0, 1)]), lambda: gpu_ctx.select_top_scale_images(100),
                     lambda: gpu_ctx.match_images([(0, 1)])):
            with pytest.raises(RuntimeError):
                call()
    finally:
        gpu_ctx.set_options(default_options())
    gpu_ctx.extract(views[:3])
    for pairs in ([(0, 3)], [(-1, 0)]):
        with pytest.raises(RuntimeError):
            gpu_ctx.prematch_images(pairs)
        with pytest.raises(RuntimeError):
            gpu_ctx.match_images(pairs)
    with pytest.raises(RuntimeError):
        gpu_ctx.prematch_images([(0, 1)], top=0)
    counts, matches = gpu_ctx.prematch_images([(0, 1)])
    assert counts[0] == len(matches[0]) >= 75
