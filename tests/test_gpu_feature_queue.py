"""The feature stages' persistent form (k_orientation_queue, k_descriptor_queue --
resident workgroups that take candidates / features from a per-extract work counter) against
SGPU_FEATURES_STATIC (grids that cover the work: k_orientation, k_descriptor_flat).  Every
candidate and feature is computed by the same code and written to the slot of its own index, so
the two forms agree bit for bit.

The contexts here are created with SGPU_WAVE_ORIENT_MAX=0 and run with
SGPU_DEBUG_DESC_WIDE_OFF: small batches then keep the quad orientation kernel and the one-wave
descriptor kernel on every call (a context otherwise gives few candidates / features the
single-image forms from its second call on, which the queue does not touch).

A wave's first unit is its index in the grid; only the units past the grid come from the
counters.  The resident grid of the device (thousands of waves) covers a small batch, so the
persistent context of most tests is created with SGPU_FEATURE_QUEUE_GRID=12: 12 one-wave
workgroups per kernel (more than the 8 counters, not a multiple of them), and every group of
candidates and every feature past the first 12 is handed out by a counter.  Every compared
extract follows an extract of other images of the same shape on the same context, which leaves
the counters advanced and other bits in the descriptor rows: a unit skipped because of a stale
counter cannot be hidden by an earlier result."""
import os

import numpy as np
import pytest

import sgpu
from sgpu_types import default_options
from sift_synth import synth_batch_fast

pytestmark = pytest.mark.gpu

C = sgpu.SiftContext
QUEUE, STATIC = C.FEATURES_QUEUE, C.FEATURES_STATIC
GRID = 12   # workgroups per kernel of the capped context


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(ctx, images, mode, flags=0):
    """(counts, keys, descriptors) of every image of one extract in the given form."""
    ctx.set_feature_queue(mode)
    ctx.set_debug_flags(C.DEBUG_DESC_WIDE_OFF | flags)
    ctx.extract(images)
    n = 1 if images.ndim == 2 else len(images)
    f = [ctx.features(i) for i in range(n)]
    return (np.array([len(k) for k, _ in f]), np.concatenate([k for k, _ in f]),
            np.concatenate([d for _, d in f]))


def _run_after(ctx, other, images, flags=0):
    """_run in the persistent form, straight after an extract of `other` on the same context."""
    _run(ctx, other, QUEUE, flags)
    return _run(ctx, images, QUEUE, flags)


def _same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and
            np.array_equal(_bits(a[2]), _bits(b[2])))


def _n_cand(ctx):
    import ctypes
    n = ctypes.c_int(0)
    sgpu.lib().sgpu_debug_candidates(ctx._ctx, None, None, 0, ctypes.byref(n))
    return n.value


@pytest.fixture(scope="module")
def ctxs(gpu_ctx):
    """(persistent form with GRID workgroups per kernel, static form, persistent form with the
    device's resident grids): contexts of their own, quad / one-wave forms kept."""
    names = ("SGPU_WAVE_ORIENT_MAX", "SGPU_FEATURE_QUEUE_GRID")
    old = {k: os.environ.get(k) for k in names}
    os.environ["SGPU_WAVE_ORIENT_MAX"] = "0"
    os.environ.pop("SGPU_FEATURE_QUEUE_GRID", None)
    try:
        s, qf = C(0, default_options(octave_num=3)), C(0, default_options(octave_num=3))
        os.environ["SGPU_FEATURE_QUEUE_GRID"] = str(GRID)
        q = C(0, default_options(octave_num=3))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield q, s, qf
    for c in (q, s, qf):
        c.close()


@pytest.fixture(scope="module")
def batch3():
    return synth_batch_fast(3, 320, 240, 8100)


@pytest.fixture(scope="module")
def other3():
    """Other images of batch3's shape: what a context extracts before a compared call."""
    return synth_batch_fast(3, 320, 240, 8150)


@pytest.fixture(scope="module")
def ref3(ctxs, batch3):
    """The static form's result of batch3, shipped descriptors (computed once, not modified)."""
    ctxs[1].set_options(default_options(octave_num=3))
    return _run(ctxs[1], batch3, STATIC)


@pytest.mark.parametrize("full_grid", [False, True])
@pytest.mark.parametrize("exact", [False, True])
def test_batch_equals_static(ctxs, batch3, other3, ref3, exact, full_grid):
    q, s, qf = ctxs
    q = qf if full_grid else q
    q.set_options(default_options(octave_num=3))
    e = C.DEBUG_EXACT_DESCRIPTOR if exact else 0
    ref = _run(s, batch3, STATIC, e) if exact else ref3
    got = _run_after(q, other3, batch3, e)
    # most groups of 16 candidates and most features lie past the capped grid's first units
    assert _n_cand(q) > 4 * 16 * GRID and ref[0].sum() > 4 * GRID, (_n_cand(q), ref[0])
    assert _same(got, ref)


def test_counters_rezeroed_between_calls(ctxs, batch3, other3, ref3):
    """The same batch twice, a batch of one, the batch again on one context: a work counter that
    is not zeroed per extract, or carries over, leaves candidates or features uncomputed."""
    q, s, _ = ctxs
    q.set_options(default_options(octave_num=3))
    one = _run(s, batch3[1], STATIC)
    assert _same(_run_after(q, other3, batch3), ref3)
    assert _same(_run(q, batch3, QUEUE), ref3)   # (a skipped candidate group changes the counts)
    assert _same(_run_after(q, other3, batch3), ref3)
    assert _same(_run_after(q, other3[0], batch3[1]), one)
    assert _same(_run_after(q, other3, batch3), ref3)
    assert one[0][0] == ref3[0][1]


@pytest.mark.parametrize("full_grid", [False, True])
def test_no_candidates(ctxs, batch3, other3, ref3, full_grid):
    """A constant image (no candidates) alone and as the middle image of a batch: the kernels
    find their counters exhausted and return."""
    q = ctxs[2] if full_grid else ctxs[0]
    q.set_options(default_options(octave_num=3))
    flat = np.full((240, 320), 128, np.uint8)
    got = _run_after(q, other3[0], flat)
    assert got[0].tolist() == [0] and _n_cand(q) == 0
    mixed = np.stack([batch3[0], flat, batch3[2]])
    got = _run_after(q, other3, mixed)
    assert got[0].tolist() == [ref3[0][0], 0, ref3[0][2]]
    keep = np.r_[0:ref3[0][0], ref3[0][0] + ref3[0][1]:ref3[0].sum()]
    assert np.array_equal(_bits(got[1]), _bits(ref3[1][keep]))
    assert np.array_equal(_bits(got[2]), _bits(ref3[2][keep]))


def test_group_boundaries_and_feature_limit(ctxs, batch3, other3):
    """Candidate counts of 16 k - 1, 16 k and 16 k + 1 (the orientation kernel takes groups of 16;
    crops of one image, searched for the counts), and a feature limit below the natural count
    (-tc: the k_limit_* kernels cap what the stages see)."""
    q, s, _ = ctxs
    for c in (q, s):
        c.set_options(default_options(octave_num=3))
    img, scrub = synth_batch_fast(2, 640, 480, 8120)   # (one 320 x 240 image: ~300 candidates)
    found = {}
    s.set_feature_queue(STATIC)
    s.set_debug_flags(C.DEBUG_DESC_WIDE_OFF)
    for h in range(480, 300, -1):
        s.extract(img[:h])
        r = _n_cand(s) % 16
        # (more groups than the capped grid's waves: a counter hands out the last, partial group)
        if r in (15, 0, 1) and r not in found and _n_cand(s) > 2 * 16 * GRID:
            found[r] = h
        if len(found) == 3:
            break
    assert sorted(found) == [0, 1, 15], found
    for r, h in found.items():
        ref = _run(s, img[:h], STATIC)
        assert _n_cand(s) % 16 == r
        assert _same(_run_after(q, scrub[:h], img[:h]), ref), (r, h)
    natural = int(_run(s, batch3[0], STATIC)[0][0])
    limit = natural // 3
    for c in (q, s):
        c.set_options(default_options(octave_num=3, feature_count_threshold=limit))
    ref = _run(s, batch3, STATIC)
    assert 0 < ref[0].max() < natural
    assert _same(_run_after(q, other3, batch3), ref)
    for c in (q, s):
        c.set_options(default_options(octave_num=3))


def test_stream_batches_own_their_counters(ctxs, other3):
    """sgpu_extract_stream keeps batches in flight side by side: each owns its set of counters,
    so the result is that of three separate extracts."""
    q, s, _ = ctxs
    for c in (q, s):
        c.set_options(default_options(octave_num=3))
    batches = [synth_batch_fast(2, 320, 240, 8200 + 10 * k) for k in range(3)]
    refs = [_run(s, b, STATIC) for b in batches]
    # (the stream's slots hold other batches' rows and advanced counters from a first pass)
    q.set_feature_queue(QUEUE)
    q.set_debug_flags(C.DEBUG_DESC_WIDE_OFF)
    q.extract_stream([other3[:2], other3[1:], other3[:2]], cap=20000)
    q.set_debug_flags(C.DEBUG_DESC_WIDE_OFF)
    k, d, c = q.extract_stream(batches, cap=sum(int(r[0].sum()) for r in refs) + 16)
    assert np.array_equal(c, np.concatenate([r[0] for r in refs]))
    assert np.array_equal(_bits(k), _bits(np.concatenate([r[1] for r in refs])))
    assert np.array_equal(_bits(d), _bits(np.concatenate([r[2] for r in refs])))


def test_fewer_features_than_waves(ctxs):
    """A 64 x 48 image: fewer groups and features than the device's resident workgroups."""
    _, s, q = ctxs
    for c in (q, s):
        c.set_options(default_options())
    img = synth_batch_fast(1, 64, 48, 8300)[0]
    ref = _run(s, img, STATIC)
    assert 0 < ref[0][0] < 2000
    assert _same(_run(q, img, QUEUE), ref)
