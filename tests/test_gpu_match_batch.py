"""The grouped pair matcher (sgpu_match_batch / sgpu_match_images) and the device quantiser
(sgpu_quantize_descriptors_gpu, sgpu_feature_descriptors_u8) on the GPU.

Expected values never come from the code under test: they are the CPU oracle's match per pair
(oracle_py.match), the per-pair gpu_ctx.match, and the host quantiser sgpu.quantize."""
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
