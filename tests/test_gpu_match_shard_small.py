"""The sharded two-set matcher at the launchers' edge sizes.

sgpu_match and sgpu_match_shard_begin run one host sequence; the shard side of it
differs in where the column side's state goes (every column's (max, row, second), merged over the
shards by sgpu_match_shard_end) and in staying on the keyed column kernels.  Small shapes whose
ties cross shard boundaries: a one-row shard, shards that end at 128 / 129 (a 128-row panel), a
257-column set 2 (one column past two 128-column tiles) and a one-column set 2; ratiomax 1.2 puts
the row side on the keyed kernel too, and lets a tied maximum pass.
"""
import numpy as np
import pytest

import oracle_py as O
import sgpu
from sift_synth import quantize, synth_descriptors

THRESHOLDS = [(0.8, 1), (1.2, 1), (0.8, 0), (1.2, 0)]


def _wide():
    """300 x 257: set 2's first 200 columns are near-copies of set 1's rows; rows of different
    shards made equal, so that their columns see a tied maximum from two shards; two equal
    columns (3 and the last one, 256) for a tied row maximum."""
    bounds = [0, 1, 128, 129, 300]
    d1 = synth_descriptors(300, 9100)
    d2 = synth_descriptors(257, 9101, base=d1, n_dup=200)
    q1, q2 = quantize(d1), quantize(d2)
    ties = [(0, 128), (5, 129), (127, 200), (60, 128 + 60)]   # (row, its copy in a later shard)
    for i, k in ties:
        q1[k] = q1[i]
    q2[256] = q2[3]
    return q1, q2, bounds, ties


def _one_column():
    """130 x 1: the column is a near-copy of row 64 (the unique maximum); rows 0 and 129, in the
    first and the last shard, are one more distant copy of it: the column's second value is tied
    between two shards."""
    bounds = [0, 1, 128, 129, 130]
    d1 = synth_descriptors(130, 9200)
    d2 = synth_descriptors(1, 9201, base=d1[64:65], n_dup=1)
    far = synth_descriptors(1, 9202, base=d1[64:65], n_dup=1, dup_noise=0.08)
    q1, q2 = quantize(d1), quantize(d2)
    q1[0] = q1[129] = quantize(far)[0]
    return q1, q2, bounds, [(0, 129)]


_CASES = {}


def _case(name):
    """The sets of a shape and the oracle's pairs for every threshold, computed once.  Checks on
    the CPU that the shape tests what it is meant to: every threshold has a match, and the
    copies' tie is decided across a shard boundary."""
    if name in _CASES:
        return _CASES[name]
    q1, q2, bounds, ties = {"wide": _wide, "one_column": _one_column}[name]()
    want = {(r, m): O.match(q1, q2, ratiomax=r, mbm=m) for r, m in THRESHOLDS}
    for w in want.values():
        assert len(w) > 0
    shard_of = lambda i: np.searchsorted(bounds, i, side="right")
    assert all(shard_of(i) != shard_of(k) for i, k in ties)
    rows = {tuple(p) for p in want[(1.2, 0)]}
    both = {tuple(p) for p in want[(1.2, 1)]}
    strict = {tuple(p) for p in want[(0.8, 1)]}
    if name == "wide":
        # both copies choose the same column; a tied maximum goes to the lower row at ratiomax
        # 1.2 and fails the ratio test at 0.8
        col = dict(rows)
        decided = [(i, k) for i, k in ties if i in col and col[i] == col.get(k)]
        assert decided
        for i, k in decided:
            assert (i, col[i]) in both and (k, col[i]) not in both
            assert (i, col[i]) not in strict and (k, col[i]) not in strict
        # the tied row maximum: one of the equal columns at 1.2 (the reference's lane order
        # picks), none at 0.8
        assert ((3, 3) in rows) != ((3, 256) in rows)
        assert 3 not in dict(tuple(p) for p in want[(0.8, 0)])
    else:
        # the tied copies are the column's second value: row 64 still wins, and would not if
        # either copy's dot counted as the maximum
        assert both == {(64, 0)} and strict == {(64, 0)}
        assert (0, 0) in rows and (129, 0) in rows
    _CASES[name] = (q1, q2, bounds, want)
    return _CASES[name]


@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["0", "DEBUG_KEYED_MATCH", "DEBUG_FUSED_MATCH"])
@pytest.mark.parametrize("ratiomax,mbm", THRESHOLDS)
@pytest.mark.parametrize("name", ["wide", "one_column"])
def test_small_shards_equal_full_and_oracle(gpu_ctx, name, ratiomax, mbm, flag):
    q1, q2, bounds, want = _case(name)
    shards = list(zip(bounds[:-1], bounds[1:]))
    try:
        gpu_ctx.set_debug_flags(0 if flag == "0" else getattr(gpu_ctx, flag))
        full = gpu_ctx.match(q1, q2, ratiomax=ratiomax, mbm=mbm)
        begun = [gpu_ctx.match_shard_begin(q1[a:b], a, q2, ratiomax=ratiomax, mbm=mbm)
                 for a, b in shards]
    finally:
        gpu_ctx.set_debug_flags(0)
    allc = np.stack([c for _, c in begun])
    got = np.concatenate([sgpu.match_shard_end(allc, r, a, ratiomax=ratiomax, mbm=mbm)
                          for (a, _), (r, _) in zip(shards, begun)])
    np.testing.assert_array_equal(got, full)
    np.testing.assert_array_equal(got, want[(ratiomax, mbm)])
