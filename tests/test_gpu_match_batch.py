"""The grouped pair matcher (sgpu_match_batch / sgpu_match_images) and the device quantiser
(sgpu_quantize_descriptors_gpu, sgpu_feature_descriptors_u8) on the GPU.

Expected values never come from the code under test: they are the CPU oracle's match per pair
(oracle_py.match), the per-pair gpu_ctx.match, and the host quantiser sgpu.quantize.

The planner gives every panel of a call ceil(4096 / total panels) column chunks of at least two
128-column tiles.  Tests 1 to 11 make calls of at most 19 pairs: every side is cut as finely as
allowed, no work item has more than two tiles and k_pairs_scan handles one pair per thread
(the chunk-limited plans).  Tests 12 to 17 reach the plans the shard workload gets (the
panel-limited ones: 1, 2 or 3 chunks per side, items of 3 to 71 tiles, 719 to 4219 pairs) by
adding thousands of filler pairs of one-row sets to the call, and prove from
SiftContext.match_plan_stats() that they ran there."""
import functools

import numpy as np
import pytest

import oracle_py as O
import sgpu
from sgpu_types import default_options
from sift_synth import quantize, synth_descriptors, synth_image, synth_tie_scene, tie_winner

pytestmark = pytest.mark.gpu


def _buffer(sets):
    """(u8 buffer, offsets) of a list of u8 sets laid back to back."""
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    buf = np.concatenate([s.reshape(-1, 128) for s in sets]) if sets else np.zeros((0, 128), np.uint8)
    return np.ascontiguousarray(buf, np.uint8), off


def _same(results, expected):
    assert len(results) == len(expected)
    for p, (r, e) in enumerate(zip(results, expected)):
        assert r.shape == e.shape and np.array_equal(r, e), (p, r.shape, e.shape)


# ---- 1: quantiser ---------------------------------------------------------------------------------

def _boundary_inputs():
    """k + 0.5 and its two float32 neighbours for k = 0 .. 299, divided by 512 (exact)."""
    h = (np.arange(300, dtype=np.float32) + np.float32(0.5))
    v = np.stack([np.nextafter(h, np.float32(-1)), h, np.nextafter(h, np.float32(1000))], 1)
    return (v.reshape(-1) / np.float32(512)).astype(np.float32)


def _rows(v):
    v = np.asarray(v, np.float32).reshape(-1)
    pad = (-len(v)) % 128
    return np.concatenate([v, np.zeros(pad, np.float32)]).reshape(-1, 128)


def test_quantize_gpu_equals_host(gpu_ctx):
    rng = np.random.Generator(np.random.PCG64(3))
    b = _boundary_inputs()
    tricky = np.float32((0.5 - 2.0 ** -25) / 512)
    assert len(b) == 900 and tricky in b
    assert np.float32(512) * tricky + np.float32(0.5) == np.float32(1.0)   # a float add rounds up
    cases = {
        "synth": synth_descriptors(1000, 7),
        "boundary": _rows(b),
        "zeros": np.zeros((3, 128), np.float32),
        "denormals": _rows(np.concatenate([np.float32(1e-45) * np.arange(1, 129, dtype=np.float32),
                                           np.full(128, 1e-39, np.float32),
                                           -np.full(128, 1e-41, np.float32)])),
        "negatives": _rows(-rng.uniform(1e-6, 0.4, 128 * 5).astype(np.float32)),
        "wrap": _rows(rng.uniform(0.0, 1.2, 128 * 9).astype(np.float32)),
    }
    for name, d in cases.items():
        want = sgpu.quantize(d)
        assert np.array_equal(want, quantize(d)), name   # the host rule itself
        assert np.array_equal(gpu_ctx.quantize_gpu(d), want), name
    got = sgpu.quantize_gpu(cases["boundary"], gpu_ctx).reshape(-1)
    assert got[int(np.where(b == tricky)[0][0])] == 0
    assert cases["wrap"].max() > 1.0 and cases["negatives"].min() < -0.3


# ---- 2: set boundaries ----------------------------------------------------------------------------

@pytest.mark.parametrize("mbm", [0, 1])
def test_columns_past_a_set_are_missing(gpu_ctx, mbm):
    """S1's last 128-column tile holds 2 real columns; the 126 rows behind them in the buffer are
    S2 = a copy of S0, which would match S0 perfectly if they leaked in."""
    d0 = synth_descriptors(257, 11)
    d1 = synth_descriptors(130, 12, base=d0, n_dup=60)
    q0, q1 = quantize(d0), quantize(d1)
    buf, off = _buffer([q0, q1, q0.copy()])
    want = O.match(q0, q1, mbm=mbm)
    assert len(want) == 60
    _same(gpu_ctx.match_batch(buf, off, [(0, 1)], mbm=mbm), [want])


# ---- 3: sizes -------------------------------------------------------------------------------------

SIZES = [0, 1, 127, 128, 129, 257, 700, 3000]
SIZE_PAIRS = ([(s, s + 1) for s in range(len(SIZES) - 1)] +
              [(3, 3), (5, 2), (2, 5), (6, 7), (6, 7), (0, 4), (4, 0), (0, 0)])


@functools.lru_cache(maxsize=None)
def _size_sets():
    sets, prev = [], None
    for s, n in enumerate(SIZES):
        dup = min(n, len(prev)) // 2 if prev is not None else 0
        d = synth_descriptors(n, 300 + s, base=prev if dup else None, n_dup=dup)
        sets.append(quantize(d))
        prev = d
    return sets


@functools.lru_cache(maxsize=None)
def _size_reference(mbm, max_match=None):
    sets = _size_sets()
    return [O.match(sets[a], sets[b], mbm=mbm, max_match=max_match) if len(sets[a]) and len(sets[b])
            else np.zeros((0, 2), np.int32) for a, b in SIZE_PAIRS]


@pytest.mark.parametrize("mbm", [0, 1])
def test_sizes_and_pair_lists(gpu_ctx, mbm):
    sets = _size_sets()
    buf, off = _buffer(sets)
    want = _size_reference(mbm)
    got = gpu_ctx.match_batch(buf, off, SIZE_PAIRS, mbm=mbm)
    _same(got, want)
    single = [gpu_ctx.match(sets[a], sets[b], mbm=mbm).copy() if len(sets[a]) and len(sets[b])
              else np.zeros((0, 2), np.int32) for a, b in SIZE_PAIRS]
    _same(got, single)
    assert sum(len(w) for w in want) > 500
    # out_counts, straight from the C call
    pr = np.ascontiguousarray(SIZE_PAIRS, np.int32)
    cap = sum(len(w) for w in want)
    out = np.zeros((cap, 2), np.int32)
    counts = np.full(len(pr), -7, np.int32)
    rc = sgpu.lib().sgpu_match_batch(gpu_ctx._ctx, buf.ctypes.data, off.ctypes.data, len(SIZES),
                                     pr.ctypes.data, len(pr), 0.7, 0.8, mbm, 3000, out.ctypes.data,
                                     cap, counts.ctypes.data, sgpu.SGPU_INPUT_HOST)
    assert rc == cap
    assert counts.tolist() == [len(w) for w in want]
    assert np.array_equal(out, np.concatenate(want))


# ---- 4: self pair ---------------------------------------------------------------------------------

def test_self_pair_is_identity(gpu_ctx):
    q = quantize(synth_descriptors(257, 11))
    want = O.match(q, q)
    assert len(want) == 257 and np.array_equal(want[:, 0], want[:, 1])
    buf, off = _buffer([quantize(synth_descriptors(40, 5)), q])
    _same(gpu_ctx.match_batch(buf, off, [(1, 1)]), [want])


# ---- 5: thresholds --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _threshold_sets():
    d1 = synth_descriptors(1500, 71)
    d2 = synth_descriptors(1800, 72, base=d1, n_dup=700)
    return quantize(synth_descriptors(77, 70)), quantize(d1), quantize(d2)


@pytest.mark.parametrize("distmax,ratiomax,mbm", [(0.7, 0.8, 1), (0.7, 0.8, 0), (0.5, 0.6, 1),
                                                  (1.0, 1.0, 0), (0.9, 0.95, 1)])
def test_thresholds(gpu_ctx, distmax, ratiomax, mbm):
    q0, q1, q2 = _threshold_sets()
    buf, off = _buffer([q0, q1, q2])
    pairs = [(1, 2), (2, 1)]
    want = [O.match(q1, q2, distmax, ratiomax, mbm), O.match(q2, q1, distmax, ratiomax, mbm)]
    assert len(want[0]) > 100
    _same(gpu_ctx.match_batch(buf, off, pairs, distmax, ratiomax, mbm), want)


# ---- 6: exact ties --------------------------------------------------------------------------------

TIE_COLS = [(200, 129), (130, 2), (4000, 33), (8999, 1), (640, 4064), (7000, 5000)]


def test_exact_ties(gpu_ctx):
    """ratiomax > 1 accepts exact ties, so the winner's index shows: RowMatch_Kernel's order on
    the row side, the first row on the column side."""
    n1, n2 = 3000, 9000
    q1, q2, rows = synth_tie_scene(n1, n2, n1 + n2, TIE_COLS, [(60, 61), (1, n1 - 5)])
    buf, off = _buffer([quantize(synth_descriptors(77, 70)), q1, q2])
    got = {}
    for mbm in (0, 1):
        got[mbm] = gpu_ctx.match_batch(buf, off, [(1, 2)], distmax=2.0, ratiomax=1.5, mbm=mbm)
        _same(got[mbm], [O.match(q1, q2, distmax=2.0, ratiomax=1.5, mbm=mbm)])
    pairs = dict(map(tuple, got[0][0].tolist()))
    assert [pairs.get(i) for i in rows] == [tie_winner(x, y) for x, y in TIE_COLS]


# ---- 7: max_match and cap -------------------------------------------------------------------------

def test_max_match_and_cap(gpu_ctx):
    sets = _size_sets()
    buf, off = _buffer(sets)
    want = _size_reference(1, 100)
    assert max(len(w) for w in want) == 100 and min(len(w) for w in want) == 0
    _same(gpu_ctx.match_batch(buf, off, SIZE_PAIRS, max_match=100), want)
    # a cap below the total: every count complete, the leading pairs that fit unchanged
    full = _size_reference(1)
    counts = [len(w) for w in full]
    total = sum(counts)
    cap = sum(counts[:6]) + counts[6] // 2
    assert counts[6] >= 2 and cap < total
    with pytest.raises(sgpu.MatchOverflow) as ei:
        gpu_ctx.match_batch(buf, off, SIZE_PAIRS, cap=cap)
    assert ei.value.counts.tolist() == counts
    _same(ei.value.matches, full[:6])
    # the C call reports SGPU_ERANGE
    pr = np.ascontiguousarray(SIZE_PAIRS, np.int32)
    out = np.zeros((cap, 2), np.int32)
    cnt = np.zeros(len(pr), np.int32)
    rc = sgpu.lib().sgpu_match_batch(gpu_ctx._ctx, buf.ctypes.data, off.ctypes.data, len(SIZES),
                                     pr.ctypes.data, len(pr), 0.7, 0.8, 1, 3000, out.ctypes.data,
                                     cap, cnt.ctypes.data, sgpu.SGPU_INPUT_HOST)
    assert rc == sgpu.SGPU_ERANGE and cnt.tolist() == counts
    assert np.array_equal(out[:sum(counts[:6])], np.concatenate(full[:6]))
    # exactly enough is no overflow
    _same(gpu_ctx.match_batch(buf, off, SIZE_PAIRS, cap=total), full)


# ---- 8: bad arguments -----------------------------------------------------------------------------

def test_bad_arguments(gpu_ctx):
    sets = _size_sets()[:4]
    buf, off = _buffer(sets)
    with pytest.raises(RuntimeError):
        gpu_ctx.match_batch(buf, off, [(1, len(sets))])
    with pytest.raises(RuntimeError):
        gpu_ctx.match_batch(buf, off, [(-1, 2)])
    bad = off.copy()
    bad[2] = bad[1] - 1
    with pytest.raises(RuntimeError):
        gpu_ctx.match_batch(buf, bad, [(1, 2)])
    assert gpu_ctx.match_batch(buf, off, []) == []
    assert gpu_ctx.match(sets[2], sets[3]) is not None   # the context still works


# ---- 9, 10, 11: extracted batches -----------------------------------------------------------------

IMAGE_PAIRS = [(0, 1), (1, 2), (2, 3), (0, 3), (3, 0)]


def _views():
    img = synth_image(320, 240, 55)
    return np.stack([np.roll(img, s, axis=(0, 1)) for s in [(0, 0), (7, 11), (3, -5), (20, 2)]])


def _check_batch(gpu_ctx):
    q = []
    for i in range(4):
        _, d = gpu_ctx.features(i)
        q.append(sgpu.quantize(d))
        assert np.array_equal(gpu_ctx.features_u8(i), q[i]), i
    got = gpu_ctx.match_images(IMAGE_PAIRS)
    _same(got, [O.match(q[a], q[b]) for a, b in IMAGE_PAIRS])
    assert min(len(g) for g in got) > 50
    return q


def test_extract_then_match_images(gpu_ctx):
    gpu_ctx.set_options(default_options())
    views = _views()
    gpu_ctx.extract(views)
    q = _check_batch(gpu_ctx)
    # the device-pointer forms over the same features
    dptr, doff = sgpu.ctypes.c_void_p(), sgpu.ctypes.c_void_p()
    u8 = sgpu.ctypes.c_void_p()
    L = sgpu.lib()
    assert L.sgpu_device_features(gpu_ctx._ctx, None, sgpu.ctypes.byref(dptr), sgpu.ctypes.byref(doff)) == 0
    assert L.sgpu_feature_descriptors_u8(gpu_ctx._ctx, sgpu.ctypes.byref(u8)) == 0 and u8.value
    total = gpu_ctx.total()
    off = np.ctypeslib.as_array(sgpu.ctypes.cast(doff, sgpu.ctypes.POINTER(sgpu.ctypes.c_int64)),
                                (5,)).copy()
    assert off[4] == total == sum(len(x) for x in q)
    pr = np.ascontiguousarray(IMAGE_PAIRS, np.int32)
    out = np.zeros((total * 2, 2), np.int32)
    cnt = np.zeros(len(pr), np.int32)
    rc = L.sgpu_match_batch(gpu_ctx._ctx, u8, off.ctypes.data, 4, pr.ctypes.data, len(pr), 0.7, 0.8, 1,
                            int(total), out.ctypes.data, len(out), cnt.ctypes.data,
                            sgpu.SGPU_INPUT_DEVICE)
    want = [O.match(q[a], q[b]) for a, b in IMAGE_PAIRS]
    assert rc == sum(len(w) for w in want) and cnt.tolist() == [len(w) for w in want]
    assert np.array_equal(out[:rc], np.concatenate(want))
    try:
        gpu_ctx.set_debug_flags(gpu_ctx.DEBUG_PARTS2)
        gpu_ctx.extract(views)
        _check_batch(gpu_ctx)
    finally:
        gpu_ctx.set_debug_flags(0)


def test_second_call_allocates_nothing(gpu_ctx):
    gpu_ctx.set_options(default_options())
    gpu_ctx.extract(_views())
    first = gpu_ctx.match_images(IMAGE_PAIRS)
    before = gpu_ctx.alloc_count()
    second = gpu_ctx.match_images(IMAGE_PAIRS)
    assert gpu_ctx.alloc_count() == before
    _same(second, first)
    assert gpu_ctx.timing()["match"] > 0


def test_match_images_error_states(gpu_ctx):
    views = _views()
    gpu_ctx.set_options(default_options())
    gpu_ctx.extract_stream([views[:2], views[2:]], cap=20000)
    gpu_ctx.batch = 4   # the binding forgets the batch too; ask the library itself
    with pytest.raises(RuntimeError):
        gpu_ctx.match_images([(0, 1)])
    with pytest.raises(RuntimeError):
        gpu_ctx.features_u8(0)
    try:
        gpu_ctx.set_options(default_options(descriptors=0))
        gpu_ctx.extract(views)
        with pytest.raises(RuntimeError):
            gpu_ctx.match_images([(0, 1)])
    finally:
        gpu_ctx.set_options(default_options())
    gpu_ctx.extract(views)
    assert len(gpu_ctx.match_images([(0, 1)])[0]) > 50


# ---- 12 to 17: the panel-limited plans ------------------------------------------------------------
#
# Filler pairs put the real pairs of a call into the plans of a call with thousands of panels: a
# pair of one-row sets costs two panels (one without mutual matching) and two trivial workgroups.

PLAN_TARGET = 4096   # kTargetItems of csrc/sift_match_plan.h: the stats assertions notice a change


@functools.lru_cache(maxsize=None)
def _filler_sets():
    """T, one row; U, one unrelated row; E, an empty set."""
    return (quantize(synth_descriptors(1, 900)), quantize(synth_descriptors(1, 901)),
            np.zeros((0, 128), np.uint8))


@functools.lru_cache(maxsize=None)
def _filler_reference(distmax, ratiomax, mbm):
    """The oracle's results of the filler pairs (T, T), (T, U) and (E, T), once each."""
    t, u, e = _filler_sets()
    for m in (0, 1):   # at the default thresholds: one match, none, none
        assert O.match(t, t, mbm=m).tolist() == [[0, 0]]
        assert len(O.match(t, u, mbm=m)) == 0 and len(O.match(e, t, mbm=m)) == 0
    return (O.match(t, t, distmax, ratiomax, mbm).copy(), O.match(t, u, distmax, ratiomax, mbm).copy(),
            O.match(e, t, distmax, ratiomax, mbm).copy())


def _positions(nreal, n):
    """List positions of nreal >= 5 real pairs in a list of n: the first, the last and, where the
    list is that long, 1023, 1024 and 1025 (the end of k_pairs_scan's first slice per thread and
    k_pairs_count's / k_pairs_write's first workgroups past 1024); the rest spread in between."""
    pos = {0, n - 1} | {p for p in (1023, 1024, 1025) if p < n}
    for p in np.linspace(1, n - 2, nreal - len(pos)).astype(int).tolist():
        while p in pos:
            p += 1
        pos.add(p)
    assert len(pos) == nreal and min(pos) == 0 and max(pos) == n - 1
    return sorted(pos)


def _mixed(real, nfill, t):
    """(pairs, src): the real pairs, in their order, spread through nfill filler pairs over the sets
    T = t, U = t + 1, E = t + 2.  The fillers alternate (T, T) and (T, U); every 64th is (E, T),
    which has no panel (an even three-way rotation would leave a third of the fillers without
    panels, and the filler counts used here would no longer reach their plans).  src[p] >= 0:
    real pair src[p]; else filler kind -1 - src[p]."""
    n = len(real) + nfill
    at = dict(zip(_positions(len(real), n), range(len(real)))) if nfill else {i: i for i in range(n)}
    kinds = [(t, t), (t, t + 1), (t + 2, t)]
    pairs, src, k = [], [], 0
    for p in range(n):
        if p in at:
            pairs.append(real[at[p]])
            src.append(at[p])
        else:
            kind = 2 if k % 64 == 63 else k % 2
            pairs.append(kinds[kind])
            src.append(-1 - kind)
            k += 1
    for p in (0, 1023, 1024, 1025, n - 1):
        assert p >= n or not nfill or src[p] >= 0
    return pairs, src


def _expected(src, real_want, fill_want):
    return [real_want[s] if s >= 0 else fill_want[-1 - s] for s in src]


def _plan_sides(pairs, sets, mbm):
    return sum(1 for a, b in pairs if len(sets[a]) and len(sets[b])) * (2 if mbm else 1)


def _c_call(gpu_ctx, buf, off, nsets, pairs, distmax, ratiomax, mbm, cap):
    """sgpu_match_batch itself: (return value, out [cap][2], counts)."""
    pr = np.ascontiguousarray(pairs, np.int32)
    out = np.zeros((max(cap, 1), 2), np.int32)
    counts = np.full(len(pr), -7, np.int32)
    rc = sgpu.lib().sgpu_match_batch(gpu_ctx._ctx, buf.ctypes.data, off.ctypes.data, nsets,
                                     pr.ctypes.data, len(pr), distmax, ratiomax, mbm, 9000,
                                     out.ctypes.data, cap, counts.ctypes.data, sgpu.SGPU_INPUT_HOST)
    return rc, out, counts


def test_plan_stats_need_a_call():
    ctx = sgpu.SiftContext(0)
    try:
        out = np.full(4, -1, np.int64)
        assert sgpu.lib().sgpu_debug_match_plan_stats(ctx._ctx, out.ctypes.data) == sgpu.SGPU_EINVAL
        assert out.tolist() == [-1] * 4
        with pytest.raises(RuntimeError):
            ctx.match_plan_stats()
        q = quantize(synth_descriptors(300, 5))
        buf, off = _buffer([q, q[:129]])
        assert len(ctx.match_batch(buf, off, [(0, 1), (1, 0)], mbm=0)) == 2
        # (0, 1): 3 panels x 1 chunk of 2 tiles; (1, 0): 2 panels x 2 chunks of 2 and 1 tiles
        assert ctx.match_plan_stats() == {"items": 7, "sides": 2, "max_tiles": 2, "max_chunks": 2}
        with pytest.raises(RuntimeError):
            ctx.match_batch(buf, off, [(0, 2)])
        with pytest.raises(RuntimeError):   # a rejected call leaves no plan
            ctx.match_plan_stats()
    finally:
        ctx.close()


# ---- 12: sizes under every plan -------------------------------------------------------------------

BIG_SIZES = [0, 1, 127, 128, 129, 257, 385, 513, 700, 897, 3000]
# the consecutive pairs, (257, 257), (513, 129), (129, 513), (897, 3000) again, (700, 385),
# (385, 700) and the empty-set pairs; ordered so that the pairs with many matches come last and
# land on the list positions from 1023 on
BIG_PAIRS = [(0, 1), (0, 4), (1, 2), (2, 3), (4, 0), (3, 4), (4, 5), (0, 0), (5, 6), (5, 5), (6, 7),
             (7, 4), (4, 7), (7, 8), (8, 6), (6, 8), (8, 9), (9, 10), (9, 10)]
# (mbm, fillers, chunks per side of the sides with enough columns): 2 * fillers (mbm 0: fillers)
# panels and the real pairs' 157 (59) leave ceil(4096 / panels) = 1, 2 or 3
BIG_PLANS = [(1, 2100, 1), (1, 1010, 2), (1, 700, 3), (0, 4200, 1), (0, 2100, 2), (0, 1400, 3)]


@functools.lru_cache(maxsize=None)
def _big_sets():
    sets, prev = [], None
    for s, n in enumerate(BIG_SIZES):
        dup = min(n, len(prev)) // 2 if prev is not None else 0
        d = synth_descriptors(n, 400 + s, base=prev if dup else None, n_dup=dup)
        sets.append(quantize(d))
        prev = d
    return sets


@functools.lru_cache(maxsize=None)
def _big_reference(mbm):
    sets = _big_sets()
    return [O.match(sets[a], sets[b], mbm=mbm).copy() if len(sets[a]) and len(sets[b])
            else np.zeros((0, 2), np.int32) for a, b in BIG_PAIRS]


def _big_call(mbm, nfill):
    """(buffer, offsets, sets, pairs, src, expected results) of BIG_PAIRS among nfill fillers."""
    sets = _big_sets() + list(_filler_sets())
    buf, off = _buffer(sets)
    pairs, src = _mixed(BIG_PAIRS, nfill, len(BIG_SIZES))
    want = _expected(src, _big_reference(mbm), _filler_reference(0.7, 0.8, mbm))
    return buf, off, sets, pairs, src, want


@pytest.mark.parametrize("mbm,nfill,chunks", BIG_PLANS)
def test_sizes_under_panel_limited_plans(gpu_ctx, mbm, nfill, chunks):
    """Every side in 1, 2 or 3 chunks: the 3000 columns of set 10 run as items of 24, 12 or 8
    tiles, the smaller sets as items of 1 to 8, and the scan sees 719 to 4219 pairs."""
    buf, off, sets, pairs, src, want = _big_call(mbm, nfill)
    real = _big_reference(mbm)
    assert len(pairs) == nfill + 19
    assert sum(len(w) for w in real) > 500
    if len(pairs) > 1025:
        assert max(len(want[p]) for p in range(1024, len(pairs)) if src[p] >= 0) > 50
    got = gpu_ctx.match_batch(buf, off, pairs, mbm=mbm)
    st = gpu_ctx.match_plan_stats()
    assert st["max_chunks"] == chunks and st["max_tiles"] == -(-24 // chunks) >= 8, st
    assert st["sides"] == _plan_sides(pairs, sets, mbm), st
    _same(got, want)
    # out_counts, straight from the C call
    cap = sum(len(w) for w in want)
    rc, out, counts = _c_call(gpu_ctx, buf, off, len(sets), pairs, 0.7, 0.8, mbm, cap)
    assert rc == cap
    assert counts.tolist() == [len(w) for w in want]
    assert np.array_equal(out, np.concatenate(want))


# ---- 13: exact ties inside one long chunk ---------------------------------------------------------

# Three columns of set 2 that copy one row of set 1 each (planted here; the first tile is the
# one of the lowest column).  RowMatch_Kernel ranks a column by col % 32 with its 5 bits reversed
# (sift_synth.tie_winner), lower first.  (101, 133, 293): the same col % 32 in three consecutive
# tiles and three 32-column blocks, so the running maximum changes in its low two bits only and
# the first tile's winner stays.  (8967, 4101, 37): 37 and 4101 share col % 32 = 5, rank 20
# (8967 % 32 is 7, rank 28, so that column loses on the first criterion); 37, in the first tile,
# survives the later equal keys.  (8965, 4069, 5): decreasing columns of one col % 32, the lowest
# in the first tile.  (67, 4129, 8806): col % 32 = 3, 1, 6 with ranks 24, 16, 12, so a later tile
# takes over twice -- but these columns belong to three lanes of the fold (a lane owns the
# columns of one col % 16), whose winners meet only in the final lane merge.  (86, 4102, 8790):
# col % 32 = 22, 6, 22 (ranks 13, 12, 13) with one col % 16, so one lane's recorded winner must
# move from the first tile to tile 32 on the rank alone (the "prefix grows" rule with an equal
# dot) and stay there in tile 68.
TIE_TRIPLES = [(101, 133, 293), (8967, 4101, 37), (8965, 4069, 5), (67, 4129, 8806),
               (86, 4102, 8790)]


@functools.lru_cache(maxsize=None)
def _tie_scene():
    n1, n2 = 3000, 9000
    row_pairs = [(60, 61), (1, n1 - 5)]
    q1, q2, rows = synth_tie_scene(n1, n2, n1 + n2, TIE_COLS, row_pairs)
    taken = {c for cs in TIE_COLS for c in cs} | {(k * 7919 + 11) % n2 for k in range(len(row_pairs))}
    assert not taken & {c for cs in TIE_TRIPLES for c in cs}
    assert len({c for cs in TIE_TRIPLES for c in cs}) == 3 * len(TIE_TRIPLES)
    busy = set(rows) | {r for rp in row_pairs for r in rp}
    rows3 = [i for i in range(100, n1) if i not in busy and
             int((q1[i].astype(np.int64) ** 2).sum()) < 262144][:len(TIE_TRIPLES)]
    for i, cs in zip(rows3, TIE_TRIPLES):
        for c in cs:
            q2[c] = q1[i]
    return q1, q2, rows, rows3


@functools.lru_cache(maxsize=None)
def _tie_reference(mbm):
    q1, q2, _, _ = _tie_scene()
    return O.match(q1, q2, distmax=2.0, ratiomax=1.5, mbm=mbm).copy()


@pytest.mark.parametrize("mbm,nfill", [(0, 4200), (1, 2100)])
def test_exact_ties_in_one_long_chunk(gpu_ctx, mbm, nfill):
    """test_exact_ties' scene as one chunk per side: direction 0 folds 71 tiles in one workgroup
    per panel, direction 1 24, so the winner's tile is kept or replaced across many loop trips."""
    q1, q2, rows, rows3 = _tie_scene()
    sets = [quantize(synth_descriptors(77, 70)), q1, q2] + list(_filler_sets())
    buf, off = _buffer(sets)
    pairs, src = _mixed([(1, 2)] * 5, nfill, 3)
    tie = _tie_reference(mbm)
    want = _expected(src, [tie] * 5, _filler_reference(2.0, 1.5, mbm))
    got = gpu_ctx.match_batch(buf, off, pairs, distmax=2.0, ratiomax=1.5, mbm=mbm)
    st = gpu_ctx.match_plan_stats()
    assert st["max_chunks"] == 1 and st["max_tiles"] == 71, st
    # one item per panel: 24 panels of set 1 over 71 tiles and, mutual, 71 panels over 24 tiles
    fill_sides = _plan_sides([p for p, s in zip(pairs, src) if s < 0], sets, mbm)
    assert st["items"] == 5 * (24 + (71 if mbm else 0)) + fill_sides, st
    _same(got, want)
    # the winners: the oracle's, which follow RowMatch_Kernel's rule for three columns too
    won = dict(map(tuple, tie.tolist()))
    assert [won.get(i) for i in rows] == [tie_winner(x, y) for x, y in TIE_COLS]
    assert [won.get(i) for i in rows3] == [tie_winner(*cs) for cs in TIE_TRIPLES]
    assert [won.get(i) for i in rows3] == [101, 37, 5, 8806, 4102]
    pr = dict(map(tuple, got[1024].tolist()))
    assert [pr.get(i) for i in rows + rows3] == [won[i] for i in rows + rows3]


# ---- 14: the cap among thousands of pairs ---------------------------------------------------------

def test_cap_among_thousands_of_pairs(gpu_ctx):
    buf, off, sets, pairs, src, full = _big_call(1, 2100)
    counts = [len(w) for w in full]
    total = sum(counts)
    k = next(p for p in range(1025, len(pairs)) if src[p] >= 0 and counts[p] >= 2)
    cap = sum(counts[:k]) + counts[k] // 2
    assert cap < total and any(src[p] >= 0 and counts[p] for p in range(k + 1, len(pairs)))
    with pytest.raises(sgpu.MatchOverflow) as ei:
        gpu_ctx.match_batch(buf, off, pairs, cap=cap)
    assert gpu_ctx.match_plan_stats()["max_chunks"] == 1
    assert ei.value.counts.tolist() == counts
    _same(ei.value.matches, full[:k])
    rc, out, cnt = _c_call(gpu_ctx, buf, off, len(sets), pairs, 0.7, 0.8, 1, cap)
    assert rc == sgpu.SGPU_ERANGE and cnt.tolist() == counts
    assert np.array_equal(out[:sum(counts[:k])], np.concatenate(full[:k]))
    # exactly enough is no overflow
    _same(gpu_ctx.match_batch(buf, off, pairs, cap=total), full)


# ---- 15: sgpu_match_images, one chunk per side ----------------------------------------------------

def _check_batch_one_chunk(gpu_ctx):
    q = [sgpu.quantize(gpu_ctx.features(i)[1]) for i in range(4)]
    n = [len(x) for x in q]
    assert min(n) > 256
    all16 = [(a, b) for a in range(4) for b in range(4)]
    panels = sum(-(-n[a] // 128) + -(-n[b] // 128) for a, b in all16)
    rep = -(-PLAN_TARGET // panels)   # the fewest repeats with ceil(4096 / total panels) = 1
    pairs = all16 * rep
    assert len(pairs) >= 200
    want = [O.match(q[a], q[b]) for a, b in all16]
    assert min(len(w) for w in want) > 50
    got = gpu_ctx.match_images(pairs)
    st = gpu_ctx.match_plan_stats()
    assert st["max_chunks"] == 1 and st["sides"] == 2 * len(pairs), st
    assert st["items"] == rep * panels and st["max_tiles"] == -(-max(n) // 128) >= 3, st
    _same(got, want * rep)


def test_match_images_one_chunk_per_side(gpu_ctx):
    """All 16 ordered pairs of four views, self pairs included, repeated until the call has 4096
    panels: every side is one chunk, as for the consecutive pairs of a shard."""
    gpu_ctx.set_options(default_options())
    views = _views()
    gpu_ctx.extract(views)
    _check_batch_one_chunk(gpu_ctx)
    try:
        gpu_ctx.set_debug_flags(gpu_ctx.DEBUG_PARTS2)
        gpu_ctx.extract(views)
        _check_batch_one_chunk(gpu_ctx)
    finally:
        gpu_ctx.set_debug_flags(0)


# ---- 16: extreme bytes at the padding edge --------------------------------------------------------

EXTREME_PAIRS = [(0, 4), (4, 0), (0, 1), (1, 0), (2, 3), (3, 2), (0, 0)]   # sets A, Z, O1, O2, S
EXTREME_THRESHOLDS = [(0.7, 0.8), (2.0, 1.0), (2.0, 1.5)]


@functools.lru_cache(maxsize=None)
def _extreme_sets():
    """A: all 255, the largest row term 128 * 128 * 255, which the column term of a padding column
    (-2^22) must still outweigh; Z: all zero; O1, O2: orthogonal half-255 rows with one planted
    copy; S: zero but for one byte of row 128, the only real column of its last tile."""
    a = np.full((300, 128), 255, np.uint8)
    z = np.zeros((129, 128), np.uint8)
    o1 = np.zeros((300, 128), np.uint8)
    o1[:, :64] = 255
    o2 = np.zeros((129, 128), np.uint8)
    o2[:, 64:] = 255
    o2[5] = o1[0]
    s = np.zeros((129, 128), np.uint8)
    s[128, 17] = 1
    return [a, z, o1, o2, s]


@functools.lru_cache(maxsize=None)
def _extreme_reference(distmax, ratiomax, mbm):
    sets = _extreme_sets()
    return [O.match(sets[a], sets[b], distmax, ratiomax, mbm).copy() for a, b in EXTREME_PAIRS]


@pytest.mark.parametrize("mbm", [0, 1])
def test_extreme_bytes_at_the_padding_edge(gpu_ctx, mbm):
    sets = _extreme_sets() + list(_filler_sets())
    buf, off = _buffer(sets)
    # the inputs decide something: (A, S) and (O1, O2) match every row at (2.0, 1.0) one way; the
    # mutual check needs an accepted tie, since all rows of A (of O1) are equal
    assert max(len(w) for w in _extreme_reference(2.0, 1.0, 0)) == 300
    assert max(len(w) for w in _extreme_reference(2.0, 1.5, mbm)) > 0
    for nfill, chunks in [(0, 2), (2100 if mbm else 4200, 1)]:
        pairs, src = _mixed(EXTREME_PAIRS, nfill, 5)
        for distmax, ratiomax in EXTREME_THRESHOLDS:
            want = _expected(src, _extreme_reference(distmax, ratiomax, mbm),
                             _filler_reference(distmax, ratiomax, mbm))
            got = gpu_ctx.match_batch(buf, off, pairs, distmax, ratiomax, mbm)
            st = gpu_ctx.match_plan_stats()
            assert st["max_chunks"] == chunks and st["max_tiles"] == (3 if nfill else 2), st
            _same(got, want)


# ---- 17: the quantiser's second grid trip ---------------------------------------------------------

def test_quantize_gpu_second_grid_trip(gpu_ctx):
    """k_quantize_desc runs at most 8192 workgroups of 256 threads, 16 bytes a thread: 262144
    descriptors a trip.  The 129 descriptors past that are the first trip's threads' second, and
    hold the rounding boundaries, wrapping and negative values of test_quantize_gpu_equals_host.
    (The kernel's s8 and row-sum outputs at this count stay covered only through match_images at
    small counts: the library has no entry point that returns them.)"""
    rng = np.random.Generator(np.random.PCG64(3))
    first = 8192 * 256 // 8
    b = _boundary_inputs()
    tricky = np.float32((0.5 - 2.0 ** -25) / 512)
    tail = np.concatenate([_rows(b), _rows(rng.uniform(0.0, 1.2, 128 * 9).astype(np.float32)),
                           _rows(-rng.uniform(1e-6, 0.4, 128 * 5).astype(np.float32))])
    assert first == 262144 and len(tail) == 22
    d = np.tile(synth_descriptors(4096, 7), (first // 4096 + 1, 1))[:first + 129].copy()
    d[first:first + len(tail)] = tail
    assert d.shape == (262144 + 129, 128) and d[first:].max() > 1.0 and d[first:].min() < -0.3
    want = sgpu.quantize(d)
    assert np.array_equal(want[first:first + len(tail)], quantize(tail))   # the host rule itself
    got = gpu_ctx.quantize_gpu(d)
    assert np.array_equal(got, want)
    at = first * 128 + int(np.where(b == tricky)[0][0])
    assert d.reshape(-1)[at] == tricky and got.reshape(-1)[at] == 0
