"""Feature tracks on the device (sgpu_tracks_batch, sgpu_tracks_images).

1  every case of tests/track_cases.py at both min_lengths: out_track, out_offsets, out_rows, the
   statistics and the return value equal the NumPy expectation exactly, a second call returns the
   same bytes, and the labels alone (out_offsets / out_rows NULL) are the same labels;
2  every SGPU_EINVAL condition leaves sentinel-filled outputs untouched and the context usable;
   a repeated call allocates nothing; times[15] is the call's and no other slot moves;
3  tracks_images after an extract of nine small images (three scenes, three rolled views each) and
   verify_images over all 36 pairs: the NumPy expectation from the downloaded matches, and
   tracks_batch on the image offsets."""
import numpy as np
import pytest

import sgpu
import track_cases as TC
from sgpu_types import default_options
from sift_synth import synth_image

gpu = pytest.mark.gpu
SENT = -9


def _c_call(ctx, case, min_length, **kw):
    """sgpu_tracks_batch itself on sentinel-filled outputs.  kw: off, nsets, pairs, npairs, matches,
    counts replace an argument (False: NULL); track / offsets / rows / stats = False pass NULL."""
    off = np.ascontiguousarray(kw.get("off", case.offsets), np.int64)
    pairs = kw.get("pairs", case.pairs)
    pairs = np.ascontiguousarray(case.pairs if pairs is False else pairs, np.int32).reshape(-1, 2)
    ms = kw.get("matches", case.matches)
    flat = None if ms is False else np.ascontiguousarray(
        np.concatenate([np.asarray(m, np.int32).reshape(-1, 2) for m in ms] + [np.zeros((0, 2), np.int32)]))
    counts = kw["counts"] if "counts" in kw else np.array([len(m) for m in case.matches], np.int32)
    counts = counts if counts is False else np.ascontiguousarray(counts, np.int32)
    rows = int(case.offsets[-1])
    outs = {"track": np.full(max(rows, 1), SENT, np.int32), "offsets": np.full(rows // 2 + 1, SENT, np.int64),
            "rows": np.full(max(rows, 1), SENT, np.int32), "stats": np.full(4, SENT, np.int64)}
    ptr = lambda a: None if a is None or a is False or a.size == 0 else a.ctypes.data
    rc = sgpu.lib().sgpu_tracks_batch(
        ctx._ctx, None if kw.get("off") is False else off.ctypes.data, kw.get("nsets", len(off) - 1),
        None if kw.get("pairs") is False else ptr(pairs), kw.get("npairs", len(pairs)), ptr(flat),
        ptr(counts), min_length,
        *(None if kw.get(k) is False else outs[k].ctypes.data for k in ("track", "offsets", "rows", "stats")))
    return rc, outs


def _untouched(outs):
    return all((a == SENT).all() for a in outs.values())


def _same(got, want, what):
    assert np.array_equal(got.track_of_row, want.track), what
    assert np.array_equal(got.offsets, want.offsets) and got.offsets.dtype == np.int64, what
    assert np.array_equal(got.rows, want.rows) and got.rows.dtype == np.int32, what
    assert np.array_equal(got.stats, want.stats), what


# ---- 1: the shared cases -----------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("min_length", TC.MIN_LENGTHS)
@pytest.mark.parametrize("name", TC.NAMES)
def test_tracks_equal_numpy(gpu_ctx, name, min_length):
    case, want = TC.cases()[name], TC.expected(name, min_length)
    rows = int(case.offsets[-1])
    rc, outs = _c_call(gpu_ctx, case, min_length)
    assert rc == want.T, (rc, sgpu.lib().sgpu_last_error(gpu_ctx._ctx))
    assert np.array_equal(outs["track"][:rows], want.track)
    assert np.array_equal(outs["offsets"][:want.T + 1], want.offsets)
    assert np.array_equal(outs["rows"][:len(want.rows)], want.rows)
    assert np.array_equal(outs["stats"], want.stats)
    # nothing past what the call owns: T + 1 offsets, offsets[T] rows
    assert (outs["offsets"][want.T + 1:] == SENT).all() and (outs["rows"][len(want.rows):] == SENT).all()
    # a second call: the same bytes
    rc2, again = _c_call(gpu_ctx, case, min_length)
    assert rc2 == rc and all(a.tobytes() == b.tobytes() for a, b in zip(outs.values(), again.values()))
    # the labels alone
    rc3, only = _c_call(gpu_ctx, case, min_length, offsets=False, rows=False, stats=False)
    assert rc3 == rc and np.array_equal(only["track"], outs["track"])
    assert (only["offsets"] == SENT).all() and (only["rows"] == SENT).all() and (only["stats"] == SENT).all()
    # the binding
    _same(gpu_ctx.tracks_batch(case.offsets, case.pairs, case.matches, min_length), want, name)


# ---- 2: refusals, allocations, timing ----------------------------------------------------------------

@gpu
def test_bad_arguments_write_nothing(gpu_ctx):
    case = TC.cases()["chain"]
    down = case.offsets.copy()
    down[3] = down[2] - 1
    neg = case.offsets.copy()
    neg[0] = -1
    huge = case.offsets.copy()
    huge[-1] = 2 ** 31
    ring = case.pairs.tolist()
    one = [[(1, 1)]] * 5
    bad = [dict(off=False), dict(nsets=-1), dict(npairs=-1), dict(off=down), dict(off=neg), dict(off=huge),
           dict(pairs=[(0, 5)] + ring[1:]), dict(pairs=[(-1, 1)] + ring[1:]), dict(pairs=False),
           dict(counts=np.array([1, -1, 1, 1, 1], np.int32)), dict(counts=False), dict(matches=False),
           dict(matches=[[(3, 1)]] + one[1:]), dict(matches=[[(1, 3)]] + one[1:]),
           dict(matches=[[(1, -1)]] + one[1:]), dict(track=False), dict(offsets=False), dict(rows=False)]
    for kw in bad:
        rc, outs = _c_call(gpu_ctx, case, 2, **kw)
        assert rc == sgpu.SGPU_EINVAL, kw
        assert _untouched(outs), kw
        assert sgpu.lib().sgpu_last_error(gpu_ctx._ctx), kw
    for ml in (1, 0, -2):
        rc, outs = _c_call(gpu_ctx, case, ml)
        assert rc == sgpu.SGPU_EINVAL and _untouched(outs), ml
    with pytest.raises(RuntimeError):
        gpu_ctx.tracks_batch(case.offsets, [(0, 5)], [[(1, 1)]])
    # the context still works
    _same(gpu_ctx.tracks_batch(case.offsets, case.pairs, case.matches), TC.expected("chain", 2), "after")


def _times(gpu_ctx, n=16):
    t = np.full(n, -1.0, np.float32)
    assert sgpu.lib().sgpu_last_timing(gpu_ctx._ctx, t.ctypes.data, n) == sgpu.SGPU_OK
    return t


@gpu
def test_allocations_and_timing(gpu_ctx):
    case, want = TC.cases()["random"], TC.expected("random", 3)
    gpu_ctx.tracks_batch(case.offsets, case.pairs, case.matches, 3)
    before = gpu_ctx.alloc_count()
    _same(gpu_ctx.tracks_batch(case.offsets, case.pairs, case.matches, 3), want, "repeat")
    small = TC.cases()["chain"]
    gpu_ctx.tracks_batch(small.offsets, small.pairs, small.matches)      # a smaller shape fits too
    assert gpu_ctx.alloc_count() == before
    t0 = _times(gpu_ctx)
    gpu_ctx.tracks_batch(case.offsets, case.pairs, case.matches, 3)
    t1 = _times(gpu_ctx)
    assert t1[15] > 0 and gpu_ctx.tracks_time() == t1[15]
    assert np.array_equal(t1[:15], t0[:15])
    assert list(gpu_ctx.timing()) == ["upload", "pyramid", "detect", "orientation", "expand",
                                      "descriptor", "download", "total", "match", "list"]


# ---- 3: tracks_images: three scenes, three rolled views each ---------------------------------------

SEEDS = [55, 56, 57]
ROLLS = [(0, 0), (7, 11), (3, -5)]   # (rows, columns) each view is rolled by
EVERY = [(a, b) for a in range(9) for b in range(a + 1, 9)]


def _views():
    return np.stack([np.roll(synth_image(320, 240, s), r, axis=(0, 1)) for s in SEEDS for r in ROLLS])


@gpu
def test_tracks_images(gpu_ctx):
    gpu_ctx.set_options(default_options())
    gpu_ctx.extract(_views())
    sizes = [gpu_ctx.count(i) for i in range(9)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    matches = gpu_ctx.verify_images(EVERY)[0]
    assert len(matches) == 36 and sum(len(m) for m in matches) > 0
    case = TC.Case(off, np.asarray(EVERY, np.int32), matches)
    for ml in TC.MIN_LENGTHS:
        want = TC.numpy_tracks(case, ml)
        got = gpu_ctx.tracks_images(EVERY, matches, ml)
        _same(got, want, ml)
        _same(gpu_ctx.tracks_batch(off, EVERY, matches, ml), want, ml)
        assert gpu_ctx.tracks_time() > 0
    # without a track through all three views of a scene this shows nothing
    want = TC.numpy_tracks(case, 3)
    lengths = np.diff(want.offsets)
    assert want.T > 0 and (lengths == 3).any(), (want.T, np.bincount(lengths))
    image, feature = sgpu.track_features(got.rows, off)
    t = int(np.flatnonzero(lengths == 3)[0])
    span = image[got.offsets[t]:got.offsets[t + 1]]
    assert len(set(span.tolist())) == 3 and len(set((span // 3).tolist())) == 1
    assert (feature >= 0).all() and (feature < np.asarray(sizes)[image]).all()
    # the error states of match_images
    with pytest.raises(RuntimeError):
        gpu_ctx.tracks_images([(0, 9)], [matches[0]])
    _same(gpu_ctx.tracks_images(EVERY, matches, 3), want, "after")
