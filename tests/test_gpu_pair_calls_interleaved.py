"""The call families over the grouped pair matcher share one host path and one set of buffers
(csrc/sgpu_pairs.cpp: b_tables, b_plan, b_part, b_dec, b_out, b_s8, b_sums).  What that can break is
one call reading another's stale size or view, so the families run interleaved on one context --
match_batch, verify_batch (H and F), prematch_batch (top = 64, with matches), match_batch_guided,
estimate_batch_refined, match_batch with a cap that overflows, then the same list reversed -- and
every result must equal, byte for byte, what the same call returns on a context of its own.  The
image side does the same over one small extracted batch.  Correctness against the oracle is the
per-family tests'; inputs: tests/pair_calls.py."""
import numpy as np
import pytest

import pair_calls as PC
import sgpu
from sgpu_types import default_options

gpu = pytest.mark.gpu


def _frozen(x):
    """A result as nested tuples of (dtype, shape, bytes): equal only if every byte is."""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (tuple, list)):
        return tuple(_frozen(v) for v in x)
    assert x is None, type(x)
    return None


def _run(call, ctx):
    try:
        return ("returned", _frozen(call(ctx)))
    except sgpu.MatchOverflow as e:
        return ("overflow", _frozen((e.counts, e.matches, getattr(e, "verified", None))))


def _alone(call, prepare=None):
    ctx = sgpu.SiftContext(0, default_options())
    try:
        if prepare:
            prepare(ctx)
        return _run(call, ctx)
    finally:
        ctx.close()


def _interleaved(calls, prepare=None):
    want = [_alone(f, prepare) for _, f in calls]
    ctx = sgpu.SiftContext(0, default_options())
    try:
        if prepare:
            prepare(ctx)
        order = list(range(len(calls))) + list(reversed(range(len(calls))))
        for step, k in enumerate(order):
            assert _run(calls[k][1], ctx) == want[k], (step, calls[k][0])
    finally:
        ctx.close()
    return want


@gpu
def test_set_calls_interleaved():
    buf, loc, scale, off, H = PC.sets()
    assert np.diff(off).tolist() == [0, 1, 130, 300, 64] and any(0 in p for p in PC.PAIRS)
    ctx = sgpu.SiftContext(0, default_options())
    try:
        putative = ctx.match_batch(buf, off, PC.PAIRS)
    finally:
        ctx.close()
    counts = [len(m) for m in putative]
    # the planted copies match, the pairs with the empty set do not, the scene matches itself
    assert counts[0] >= 40 and counts[2] >= 25 and counts[5] == counts[6] == 0 and counts[7] == 300
    cap = sum(counts[:3]) + counts[3] // 2   # ends inside the fourth pair
    assert 0 < cap < sum(counts)
    want = _interleaved(PC.set_calls(putative, cap))
    assert [w[0] for w in want] == ["returned"] * 5 + ["overflow"]
    assert want[0][1] == _frozen(putative)
    assert len(want[5][1][1]) == 3   # the prefix that fits: three pairs


@gpu
def test_image_calls_interleaved():
    def extract(ctx):
        ctx.extract(PC.views())
        assert min(ctx.count(i) for i in range(len(PC.ROLLS))) > 0

    want = _interleaved(PC.image_calls(), extract)
    assert [w[0] for w in want] == ["returned"] * 4
    matches = want[0][1]
    assert len(matches) == len(PC.IMAGE_PAIRS) and all(m[1][0] > 0 for m in matches)
