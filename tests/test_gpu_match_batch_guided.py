"""Guided matching in the grouped pair matcher (sgpu_match_batch_guided /
sgpu_match_images_guided): many set pairs in one call, each under its own H and F.

Expected values never come from the code under test: they are the CPU oracle's guided match per
pair (oracle_py.match_guided) and the single-pair gpu_ctx.match_guided per pair.  Every scene's
oracle result is checked first, on the CPU, to be non-trivial (the geometry removes some but
not all of the plain matches), so that an accept-all or reject-all kernel cannot pass.

The planner is the plain matcher's (test_gpu_match_batch.py's docstring): calls of a few pairs
are cut as finely as allowed (the chunk-limited plans); test 5 adds filler pairs of one-row sets
until every side is 1, 2 or 3 chunks of many tiles (the panel-limited plans) and proves the
regime with SiftContext.match_plan_stats()."""
import functools

import numpy as np
import pytest

import oracle_py as O
import sgpu
from sgpu_types import default_options
from sift_synth import (quantize, synth_descriptors, synth_guided_scene, synth_image,
                        synth_tie_scene, tie_winner)

gpu = pytest.mark.gpu
NONE = np.zeros((0, 2), np.int32)
EYE = np.eye(3, dtype=np.float32)


def _buffer(sets):
    """(u8 buffer, locations, offsets) of a list of (descriptors, locations) laid back to back."""
    off = np.concatenate([[0], np.cumsum([len(q) for q, _ in sets])]).astype(np.int64)
    buf = np.concatenate([q.reshape(-1, 128) for q, _ in sets])
    loc = np.concatenate([l.reshape(-1, 2) for _, l in sets])
    return np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(loc, np.float32), off


def _same(results, expected):
    assert len(results) == len(expected)
    for p, (r, e) in enumerate(zip(results, expected)):
        assert r.shape == e.shape and np.array_equal(r, e), (p, r.shape, e.shape)


def _oracle(sets, pairs, Hs, Fs, **kw):
    """The oracle's guided match of every pair under its own matrices (None: that matrix is
    missing for all pairs)."""
    out = []
    for p, (a, b) in enumerate(pairs):
        (qa, la), (qb, lb) = sets[a], sets[b]
        if len(qa) == 0 or len(qb) == 0:
            out.append(NONE)
            continue
        out.append(O.match_guided(qa, qb, la, lb, None if Hs is None else Hs[p],
                                  None if Fs is None else Fs[p], **kw).copy())
    return out


def _single(gpu_ctx, sets, pairs, Hs, Fs, **kw):
    """The same from the single-pair matcher, one call per pair."""
    out = []
    for p, (a, b) in enumerate(pairs):
        (qa, la), (qb, lb) = sets[a], sets[b]
        if len(qa) == 0 or len(qb) == 0:
            out.append(NONE)
            continue
        out.append(gpu_ctx.match_guided(qa, qb, la, lb, None if Hs is None else Hs[p],
                                        None if Fs is None else Fs[p], **kw).copy())
    return out


def _c_call(gpu_ctx, buf, loc, off, nsets, pairs, Hs, Fs, mbm, max_match, cap, **th):
    """sgpu_match_batch_guided itself: (return value, out [cap][2], counts)."""
    pr = np.ascontiguousarray(pairs, np.int32)
    out = np.zeros((max(cap, 1), 2), np.int32)
    counts = np.full(len(pr), -7, np.int32)
    hm = None if Hs is None else np.ascontiguousarray(Hs, np.float32).reshape(len(pr), 9)
    fm = None if Fs is None else np.ascontiguousarray(Fs, np.float32).reshape(len(pr), 9)
    rc = sgpu.lib().sgpu_match_batch_guided(
        gpu_ctx._ctx, buf.ctypes.data, None if loc is None else loc.ctypes.data, off.ctypes.data,
        nsets, pr.ctypes.data, len(pr), None if hm is None else hm.ctypes.data,
        None if fm is None else fm.ctypes.data, th.get("distmax", 0.7), th.get("ratiomax", 0.8),
        th.get("hdistmax", 32.0), th.get("fdistmax", 16.0), mbm, max_match, out.ctypes.data, cap,
        counts.ctypes.data, sgpu.SGPU_INPUT_HOST)
    return rc, out, counts


# ---- 1, 2: sizes, pair lists and which matrices ---------------------------------------------------

# five independent scenes laid back to back: scene k = sets 2k (set 1) and 2k + 1 (set 2); then a
# one-row set and an empty set.  Sizes 129, 257, 300, 127, 700, 128, 257, 300, 9, 7, 1, 0.
SCENES = [(129, 257, 21), (300, 127, 22), (700, 128, 23), (257, 300, 24), (9, 7, 25)]
PLANTED = 4   # the scenes large enough for planted matches that the geometry thins out
ONE, EMPTY = 10, 11
# (pair, scene whose H and F it runs under): every scene's own pair; a cross-scene pair (unrelated
# geometry); (a, a); a repeated pair; a pair in both orders; the one-row set; the empty set
SCENE_PAIRS = [((0, 1), 0), ((2, 3), 1), ((4, 5), 2), ((6, 7), 3), ((8, 9), 4),
               ((0, 3), 0), ((4, 4), 2), ((2, 3), 1), ((1, 0), 0), ((7, 6), 3),
               ((ONE, 1), 0), ((5, ONE), 2), ((EMPTY, 0), 0), ((0, EMPTY), 0), ((EMPTY, EMPTY), 1)]
PAIRS = [p for p, _ in SCENE_PAIRS]


@functools.lru_cache(maxsize=None)
def _scene_sets():
    sets, Hs, Fs = [], [], []
    for n1, n2, seed in SCENES:
        q1, q2, l1, l2, H, F = synth_guided_scene(n1, n2, seed)
        sets += [(q1, l1), (q2, l2)]
        Hs.append(H)
        Fs.append(F)
    sets.append((quantize(synth_descriptors(1, 31)), np.array([[100.0, 200.0]], np.float32)))
    sets.append((np.zeros((0, 128), np.uint8), np.zeros((0, 2), np.float32)))
    assert sorted({len(q) for q, _ in sets}) == [0, 1, 7, 9, 127, 128, 129, 257, 300, 700]
    pH = np.stack([Hs[s] for _, s in SCENE_PAIRS])
    pF = np.stack([Fs[s] for _, s in SCENE_PAIRS])
    return sets, pH, pF


@functools.lru_cache(maxsize=None)
def _scene_reference(mbm, use_h=True, use_f=True, hdistmax=32.0, fdistmax=16.0):
    sets, pH, pF = _scene_sets()
    return _oracle(sets, PAIRS, pH if use_h else None, pF if use_f else None, mbm=mbm,
                   hdistmax=hdistmax, fdistmax=fdistmax)


def _nontrivial(guided, plain):
    """The geometry removed some of the plain matches of every planted scene, and kept some."""
    for k in range(PLANTED):
        assert 0 < len(guided[k]) < len(plain[k]), (k, len(guided[k]), len(plain[k]))


@gpu
@pytest.mark.parametrize("mbm", [0, 1])
def test_sizes_and_pair_lists(gpu_ctx, mbm):
    sets, pH, pF = _scene_sets()
    want = _scene_reference(mbm)
    plain = _scene_reference(mbm, False, False)
    _nontrivial(want, plain)
    # the oracle finds 298 matches over the list (1277 without geometry)
    assert sum(len(w) for w in want) > 250
    assert len(want[5]) < 5 and np.array_equal(want[1], want[7])   # cross-scene; the repeat
    buf, loc, off = _buffer(sets)
    got = gpu_ctx.match_batch_guided(buf, loc, off, PAIRS, pH, pF, mbm=mbm)
    _same(got, want)
    _same(got, _single(gpu_ctx, sets, PAIRS, pH, pF, mbm=mbm))
    # out_counts, straight from the C call
    cap = sum(len(w) for w in want)
    rc, out, counts = _c_call(gpu_ctx, buf, loc, off, len(sets), PAIRS, pH, pF, mbm, 9000, cap)
    assert rc == cap and counts.tolist() == [len(w) for w in want]
    assert np.array_equal(out, np.concatenate(want))


@gpu
@pytest.mark.parametrize("use_h,use_f", [(True, True), (True, False), (False, True)])
def test_which_matrices(gpu_ctx, use_h, use_f):
    """Tight thresholds (hdistmax 8, fdistmax 1); a missing array is the identity at 1e20."""
    sets, pH, pF = _scene_sets()
    want = _scene_reference(1, use_h, use_f, 8.0, 1.0)
    _nontrivial(want, _scene_reference(1, False, False))
    buf, loc, off = _buffer(sets)
    H, F = pH if use_h else None, pF if use_f else None
    got = gpu_ctx.match_batch_guided(buf, loc, off, PAIRS, H, F, hdistmax=8.0, fdistmax=1.0)
    _same(got, want)
    _same(got, _single(gpu_ctx, sets, PAIRS, H, F, hdistmax=8.0, fdistmax=1.0))


@gpu
def test_no_matrices_is_match_batch(gpu_ctx):
    sets, _, _ = _scene_sets()
    buf, loc, off = _buffer(sets)
    want = _scene_reference(1, False, False)
    assert sum(len(w) for w in want) > 500
    got = gpu_ctx.match_batch_guided(buf, loc, off, PAIRS, None, None)
    _same(got, want)
    _same(got, gpu_ctx.match_batch(buf, off, PAIRS))
    # the locations are not read
    total = sum(len(w) for w in want)
    rc, out, counts = _c_call(gpu_ctx, buf, None, off, len(sets), PAIRS, None, None, 1, 9000, total)
    assert rc == total and np.array_equal(out, np.concatenate(want))


# ---- 3: the block rule at an unaligned set --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _block_rule_scene():
    """test_match_guided_block_rule's planted case: row r's descriptor sits at column j, where r
    itself fails the geometric test and only its block mate passes."""
    q1, q2, l1, l2, H, F = synth_guided_scene(64, 40, 9, n_dup=0)
    self_dot = (q1.astype(np.int64) ** 2).sum(1)
    r = int(next(i for i in range(1, 64) if self_dot[i] > 262144 and i % 8))
    mate, j = r - r % 8 + (0 if r % 8 else 1), 17
    q2[j] = q1[r]
    x = H.astype(np.float64) @ np.array([l1[mate, 0], l1[mate, 1], 1.0])
    l2[j] = (x[:2] / x[2]).astype(np.float32)
    return q1, q2, l1, l2, H, F, r, j


@gpu
def test_block_rule_at_an_unaligned_set(gpu_ctx):
    """Five rows in front put set 1 at buffer row 5: the 8-row blocks of MultiplyDescriptorG_Kernel
    count from the set's first row, not the buffer's."""
    q1, q2, l1, l2, H, F, r, j = _block_rule_scene()
    front = (quantize(synth_descriptors(5, 61)), np.full((5, 2), 300.0, np.float32))
    sets = [front, (q1, l1), (q2, l2)]
    buf, loc, off = _buffer(sets)
    assert off[1] % 8 == 5
    for dm, rm, mbm in ((2.0, 1.0, 0), (2.0, 1.0, 1), (0.7, 0.8, 1)):
        want = O.match_guided(q1, q2, l1, l2, H, F, distmax=dm, ratiomax=rm, mbm=mbm).copy()
        got = gpu_ctx.match_batch_guided(buf, loc, off, [(1, 2)], H[None], F[None], distmax=dm,
                                         ratiomax=rm, mbm=mbm)
        _same(got, [want])
        _same(got, [gpu_ctx.match_guided(q1, q2, l1, l2, H, F, distmax=dm, ratiomax=rm, mbm=mbm)])
        if mbm == 0:
            assert [r, j] in got[0].tolist()


# ---- 4: neighbouring sets do not leak -------------------------------------------------------------

@gpu
@pytest.mark.parametrize("mbm", [0, 1])
def test_neighbouring_sets_do_not_leak(gpu_ctx, mbm):
    """Set b's last 128-column tile holds 2 real columns; the 126 rows behind them in the buffer
    are a copy of set a, descriptors and locations, which would match set a perfectly under
    H = identity if either leaked in.  (Direction 1 has the same layout: set a's last tile holds
    one real column and set b lies behind it.)"""
    d0 = synth_descriptors(257, 11)
    d1 = synth_descriptors(130, 12, base=d0, n_dup=60)
    q0, q1 = quantize(d0), quantize(d1)
    rng = np.random.Generator(np.random.PCG64(13))
    l0 = rng.uniform(0, 1000, (257, 2)).astype(np.float32)
    l1 = rng.uniform(0, 1000, (130, 2)).astype(np.float32)
    l1[:60] = l0[:60]
    l1[2:60:3] += 500.0   # descriptor matches the geometry must reject
    sets = [(q0, l0), (q1, l1), (q0.copy(), l0.copy())]
    want = O.match_guided(q0, q1, l0, l1, EYE, None, hdistmax=4.0, mbm=mbm).copy()
    plain = O.match(q0, q1, mbm=mbm)
    assert len(plain) == 60 and len(want) == 40
    buf, loc, off = _buffer(sets)
    _same(gpu_ctx.match_batch_guided(buf, loc, off, [(0, 1)], EYE[None], None, hdistmax=4.0,
                                     mbm=mbm), [want])


# ---- 5: panel-limited plans -----------------------------------------------------------------------

BIG = (3000, 2100, 33)
BIG_REAL = [(0, 1), (1, 0), (0, 1)]
# (mbm, fillers, chunks per side): the real pairs' panels (mutual: 41 each) and one panel per side
# of every filler leave ceil(4096 / panels) = 1, 2 or 3
BIG_PLANS = [(1, 2100, 1), (1, 1010, 2), (1, 700, 3), (0, 2100, 2)]
# a skew-symmetric F: x' F x = 0, so a filler pair at one location has no Sampson error
SKEW = np.array([[0, -1.0, 0.5], [1.0, 0, -0.3], [-0.5, 0.3, 0]], np.float32)


@functools.lru_cache(maxsize=None)
def _big_sets():
    q1, q2, l1, l2, H, F = synth_guided_scene(*BIG)
    t = quantize(synth_descriptors(1, 900))
    u = quantize(synth_descriptors(1, 901))
    at = np.array([[640.0, 360.0]], np.float32)
    return [(q1, l1), (q2, l2), (t, at), (u, at.copy())], H, F


@functools.lru_cache(maxsize=None)
def _big_reference(mbm):
    sets, H, F = _big_sets()
    real = _oracle(sets, BIG_REAL[:2], [H, H], [F, F], mbm=mbm)
    fill = _oracle(sets, [(2, 2), (2, 3)], [EYE, EYE], [SKEW, SKEW], mbm=mbm)
    # the fillers' geometry accepts: (T, T) matches, (T, U) does not (its descriptors differ)
    assert fill[0].tolist() == [[0, 0]] and len(fill[1]) == 0
    return real + [real[0]], fill


def _with_fillers(nfill):
    """The real pairs first, last and in the middle of nfill fillers alternating (T, T), (T, U)."""
    n = nfill + len(BIG_REAL)
    at = {0: 0, n // 2: 1, n - 1: 2}
    pairs, src, k = [], [], 0
    for p in range(n):
        if p in at:
            pairs.append(BIG_REAL[at[p]])
            src.append(at[p])
        else:
            pairs.append((2, 2 + k % 2))
            src.append(-1 - k % 2)
            k += 1
    return pairs, src


@gpu
@pytest.mark.parametrize("mbm,nfill,chunks", BIG_PLANS)
def test_panel_limited_plans(gpu_ctx, mbm, nfill, chunks):
    """A 3000 x 2100 scene among fillers: every side is 1, 2 or 3 chunks, the 3000 columns run as
    items of 24, 12 or 8 tiles, so the guided tile loop makes many trips per work item."""
    sets, H, F = _big_sets()
    real, fill = _big_reference(mbm)
    plain = O.match(sets[0][0], sets[1][0], mbm=mbm)
    assert 0 < len(real[0]) < len(plain) and len(real[0]) > 500
    pairs, src = _with_fillers(nfill)
    want = [real[s] if s >= 0 else fill[-1 - s] for s in src]
    pH = np.stack([H if s >= 0 else EYE for s in src])
    pF = np.stack([F if s >= 0 else SKEW for s in src])
    buf, loc, off = _buffer(sets)
    got = gpu_ctx.match_batch_guided(buf, loc, off, pairs, pH, pF, mbm=mbm)
    st = gpu_ctx.match_plan_stats()
    assert st["max_chunks"] == chunks and st["max_tiles"] == -(-24 // chunks) >= 8, st
    assert st["sides"] == len(pairs) * (2 if mbm else 1), st
    _same(got, want)


# ---- 6: exact ties under geometry -----------------------------------------------------------------

TIE_COLS = [(5, 37), (130, 2), (200, 456), (64, 640), (77, 301)]
# which of the two tied columns lies where the geometry accepts it: 0, 1, or 2 = both
TIE_PASS = [1, 0, 2, 1, 2]
TIE_ROWS = [(60, 61), (1, 295)]   # rows of set 1 that copy one column of set 2; the second passes


@functools.lru_cache(maxsize=None)
def _tie_scene():
    n1, n2 = 300, 700
    q1, q2, rows = synth_tie_scene(n1, n2, 1000, TIE_COLS, TIE_ROWS)
    rng = np.random.Generator(np.random.PCG64(14))
    l1 = rng.uniform(0, 1000, (n1, 2)).astype(np.float32)
    l2 = rng.uniform(2000, 3000, (n2, 2)).astype(np.float32)   # nothing passes unless placed
    for i, cols, ok in zip(rows, TIE_COLS, TIE_PASS):
        for k, c in enumerate(cols):
            if ok in (k, 2):
                l2[c] = l1[i]
    for k, (ra, rb) in enumerate(TIE_ROWS):
        l2[(k * 7919 + 11) % n2] = l1[rb]
    return q1, q2, l1, l2, rows


@gpu
@pytest.mark.parametrize("mbm", [0, 1])
def test_exact_ties_under_geometry(gpu_ctx, mbm):
    """Two columns tie on the dot; where one of them fails the geometric test the other wins,
    whatever the tie order says, and where both pass RowMatch_Kernel's order decides.  The same on
    the column side: of two tied rows of set 1 the one that passes is the column's match."""
    q1, q2, l1, l2, rows = _tie_scene()
    kw = dict(distmax=2.0, ratiomax=1.5, hdistmax=8.0, mbm=mbm)
    want = O.match_guided(q1, q2, l1, l2, EYE, None, **kw).copy()
    won = dict(map(tuple, want.tolist()))
    expect = [tie_winner(*cs) if ok == 2 else cs[ok] for cs, ok in zip(TIE_COLS, TIE_PASS)]
    assert [won.get(i) for i in rows] == expect
    assert expect[0] != tie_winner(*TIE_COLS[0]) and expect[1] != tie_winner(*TIE_COLS[1])
    # (without the mutual check row 60 still matches: its block mate 61 passes, the block rule)
    for k, (ra, rb) in enumerate(TIE_ROWS):
        assert won.get(rb) == (k * 7919 + 11) % 700 and (ra not in won or not mbm)
    sets = [(quantize(synth_descriptors(3, 70)), np.zeros((3, 2), np.float32)), (q1, l1), (q2, l2)]
    buf, loc, off = _buffer(sets)
    got = gpu_ctx.match_batch_guided(buf, loc, off, [(1, 2)], EYE[None], None, **kw)
    _same(got, [want])
    _same(got, [gpu_ctx.match_guided(q1, q2, l1, l2, EYE, None, **kw)])


# ---- 7: extract, then match_images_guided ---------------------------------------------------------

ROLLS = [(0, 0), (7, 11), (3, -5), (20, 2)]   # (rows, columns) each view is rolled by
IMAGE_PAIRS = [(0, 1), (1, 2), (2, 3), (0, 3), (3, 0)]


def _views():
    img = synth_image(320, 240, 55)
    return np.stack([np.roll(img, s, axis=(0, 1)) for s in ROLLS])


def _roll_geometry():
    """H_p = the translation that takes view a's features to view b's; F_p = [e]_x H_p."""
    Hs, Fs = [], []
    e = np.array([0.4, -0.7, 1e-3])
    ex = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
    for a, b in IMAGE_PAIRS:
        H = np.eye(3)
        H[0, 2] = ROLLS[b][1] - ROLLS[a][1]
        H[1, 2] = ROLLS[b][0] - ROLLS[a][0]
        F = ex @ H
        Hs.append(H.astype(np.float32))
        Fs.append((F / np.linalg.norm(F)).astype(np.float32))
    return np.stack(Hs), np.stack(Fs)


def _check_images(gpu_ctx):
    keys, q = [], []
    for i in range(4):
        k, _ = gpu_ctx.features(i)
        keys.append(np.ascontiguousarray(k[:, :2], np.float32))
        q.append(gpu_ctx.features_u8(i))
    sets = list(zip(q, keys))
    pH, pF = _roll_geometry()
    plain = [O.match(q[a], q[b]) for a, b in IMAGE_PAIRS]
    for F in (None, pF):
        want = _oracle(sets, IMAGE_PAIRS, pH, F, hdistmax=3.0, fdistmax=1.0)
        assert min(len(w) for w in want) > 50
        # the geometry decides: it removes rivals in the ratio test as well as matches, so the
        # counts may grow, but the results are not the plain ones
        assert any(not np.array_equal(w, p) for w, p in zip(want, plain))
        got = gpu_ctx.match_images_guided(IMAGE_PAIRS, pH, F, hdistmax=3.0, fdistmax=1.0)
        _same(got, want)
        _same(got, _single(gpu_ctx, sets, IMAGE_PAIRS, pH, F, hdistmax=3.0, fdistmax=1.0))
    _same(gpu_ctx.match_images_guided(IMAGE_PAIRS), plain)


@gpu
def test_extract_then_match_images_guided(gpu_ctx):
    gpu_ctx.set_options(default_options())
    views = _views()
    gpu_ctx.extract(views)
    _check_images(gpu_ctx)
    try:
        gpu_ctx.set_debug_flags(gpu_ctx.DEBUG_PARTS2)
        gpu_ctx.extract(views)
        _check_images(gpu_ctx)
    finally:
        gpu_ctx.set_debug_flags(0)


# ---- 8: bookkeeping -------------------------------------------------------------------------------

@gpu
def test_second_call_allocates_nothing(gpu_ctx):
    sets, pH, pF = _scene_sets()
    buf, loc, off = _buffer(sets)
    first = gpu_ctx.match_batch_guided(buf, loc, off, PAIRS, pH, pF)
    before = gpu_ctx.alloc_count()
    second = gpu_ctx.match_batch_guided(buf, loc, off, PAIRS, pH, pF)
    assert gpu_ctx.alloc_count() == before
    _same(second, first)
    assert gpu_ctx.timing()["match"] > 0
    gpu_ctx.set_options(default_options())
    gpu_ctx.extract(_views())
    pH, pF = _roll_geometry()
    first = gpu_ctx.match_images_guided(IMAGE_PAIRS, pH, pF)
    before = gpu_ctx.alloc_count()
    _same(gpu_ctx.match_images_guided(IMAGE_PAIRS, pH, pF), first)
    assert gpu_ctx.alloc_count() == before
    assert gpu_ctx.timing()["match"] > 0


@gpu
def test_max_match_and_cap(gpu_ctx):
    sets, pH, pF = _scene_sets()
    buf, loc, off = _buffer(sets)
    full = _scene_reference(1)
    lim = _oracle(sets, PAIRS, pH, pF, mbm=1, max_match=10)
    assert max(len(w) for w in full) > 10 and [len(w) for w in lim] == [min(len(w), 10) for w in full]
    _same(gpu_ctx.match_batch_guided(buf, loc, off, PAIRS, pH, pF, max_match=10), lim)
    counts = [len(w) for w in full]
    k = 3   # the cap ends inside pair 3
    cap = sum(counts[:k]) + counts[k] // 2
    assert counts[k] >= 2 and sum(counts[k + 1:]) > 0
    with pytest.raises(sgpu.MatchOverflow) as ei:
        gpu_ctx.match_batch_guided(buf, loc, off, PAIRS, pH, pF, cap=cap)
    assert ei.value.counts.tolist() == counts
    _same(ei.value.matches, full[:k])
    rc, out, cnt = _c_call(gpu_ctx, buf, loc, off, len(sets), PAIRS, pH, pF, 1, 9000, cap)
    assert rc == sgpu.SGPU_ERANGE and cnt.tolist() == counts
    assert np.array_equal(out[:sum(counts[:k])], np.concatenate(full[:k]))
    _same(gpu_ctx.match_batch_guided(buf, loc, off, PAIRS, pH, pF, cap=sum(counts)), full)


@gpu
def test_bad_arguments(gpu_ctx):
    sets, pH, pF = _scene_sets()
    buf, loc, off = _buffer(sets)
    with pytest.raises(RuntimeError):
        gpu_ctx.match_batch_guided(buf, loc, off, [(1, len(sets))], pH[:1], pF[:1])
    with pytest.raises(RuntimeError):
        gpu_ctx.match_batch_guided(buf, loc, off, [(-1, 2)], pH[:1], None)
    rc, _, _ = _c_call(gpu_ctx, buf, loc, off, len(sets), [(0, len(sets))], pH[:1], pF[:1], 1, 9000, 100)
    assert rc == sgpu.SGPU_EINVAL
    rc, _, _ = _c_call(gpu_ctx, buf, None, off, len(sets), [(0, 1)], pH[:1], None, 1, 9000, 100)
    assert rc == sgpu.SGPU_EINVAL   # a matrix needs locations
    assert gpu_ctx.match_batch_guided(buf, loc, off, [], None, None) == []
    _same(gpu_ctx.match_batch_guided(buf, loc, off, PAIRS[:1], pH[:1], pF[:1]), _scene_reference(1)[:1])


@gpu
def test_match_images_guided_error_states(gpu_ctx):
    views = _views()
    pH, pF = _roll_geometry()
    gpu_ctx.set_options(default_options())
    gpu_ctx.extract_stream([views[:2], views[2:]], cap=20000)
    gpu_ctx.batch = 4   # the binding forgets the batch too; ask the library itself
    with pytest.raises(RuntimeError):
        gpu_ctx.match_images_guided([(0, 1)], pH[:1], pF[:1])
    try:
        gpu_ctx.set_options(default_options(descriptors=0))
        gpu_ctx.extract(views)
        with pytest.raises(RuntimeError):
            gpu_ctx.match_images_guided([(0, 1)], pH[:1], None)
    finally:
        gpu_ctx.set_options(default_options())
    gpu_ctx.extract(views)
    with pytest.raises(RuntimeError):
        gpu_ctx.match_images_guided([(0, 4)], pH[:1], None)
    assert len(gpu_ctx.match_images_guided([(0, 1)], pH[:1], pF[:1])[0]) > 50


def test_binding_rejects_wrong_shapes():
    """The binding's ValueErrors come before any C call: no device, no library needed."""
    ctx = sgpu.SiftContext.__new__(sgpu.SiftContext)
    ctx._ctx = None
    q = np.zeros((10, 128), np.uint8)
    loc = np.zeros((10, 2), np.float32)
    off = [0, 4, 10]
    pairs = [(0, 1), (1, 0)]
    H2 = np.stack([EYE, EYE])
    for bad in (np.zeros((10, 4), np.float32), np.zeros((9, 2), np.float32), np.zeros(20, np.float32)):
        with pytest.raises(ValueError):
            ctx.match_batch_guided(q, bad, off, pairs, H2, None)
    for bad in (EYE, np.stack([EYE] * 3), np.zeros((2, 2, 3), np.float32), np.zeros(18, np.float32)):
        with pytest.raises(ValueError):
            ctx.match_batch_guided(q, loc, off, pairs, bad, None)
        with pytest.raises(ValueError):
            ctx.match_batch_guided(q, loc, off, pairs, H2, bad)
        with pytest.raises(ValueError):
            ctx.match_images_guided(pairs, bad, None)
        with pytest.raises(ValueError):
            ctx.match_images_guided(pairs, None, bad)
