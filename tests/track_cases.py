"""Cases and the NumPy reference of the track rule (csrc/sift_tracks.h), shared by the CPU test of
sgtrk::tracks_host (tests/test_tracks.py) and the GPU test of sgpu_tracks_batch
(tests/test_gpu_tracks.py).

The expected values come from NumPy alone and know nothing of union-find: every row starts with its
own index as label, the minimum label is propagated over the edges (and along label -> label of
label) until nothing changes, and the components are then grouped, tested and numbered by the rule.
Every case is seeded; the expectations are computed once per (case, min_length) and shared."""
from __future__ import annotations

import collections
import functools

import numpy as np

NONE, INCONSISTENT = -1, -2
MIN_LENGTHS = (2, 3)

Case = collections.namedtuple("Case", "offsets pairs matches")          # int64, [n, 2] int32, list of [m, 2]
Expected = collections.namedtuple("Expected", "track offsets rows stats T")


def _case(sizes, pairs, matches):
    off = np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int64)
    pr = np.asarray(pairs, np.int32).reshape(-1, 2)
    ms = [np.asarray(m, np.int32).reshape(-1, 2) for m in matches]
    assert len(ms) == len(pr)
    return Case(off, pr, ms)


def edges(case: Case):
    """The rows (u, v) of every match, in pair order."""
    u = [case.offsets[a] + m[:, 0] for (a, _), m in zip(case.pairs, case.matches)]
    v = [case.offsets[b] + m[:, 1] for (_, b), m in zip(case.pairs, case.matches)]
    cat = lambda parts: np.concatenate(parts + [np.zeros(0, np.int64)]).astype(np.int64)
    return cat(u), cat(v)


def numpy_tracks(case: Case, min_length: int) -> Expected:
    off = case.offsets
    rows, nsets = int(off[-1]), len(off) - 1
    u, v = edges(case)
    label = np.arange(rows, dtype=np.int64)
    while True:   # the minimum label over the edges, to a fixed point
        new = label.copy()
        np.minimum.at(new, u, label[v])
        np.minimum.at(new, v, label[u])
        new = new[new]
        if np.array_equal(new, label):
            break
        label = new
    size = np.bincount(label, minlength=rows)
    r = np.arange(rows, dtype=np.int64)
    root = label == r
    n = np.where(root, size, 0)
    short = root & (n >= 2) & (n < min_length)
    oversize = root & (n >= 2) & (n >= min_length) & (n > nsets)
    cand = root & (n >= 2) & (n >= min_length) & (n <= nsets)
    # two rows of a candidate in one set
    set_of = np.searchsorted(off, r, side="right") - 1
    in_cand = cand[label]
    key, cnt = np.unique(label[in_cand] * max(nsets, 1) + set_of[in_cand], return_counts=True)
    twice = np.zeros(rows, bool)
    twice[key[cnt > 1] // max(nsets, 1)] = True
    good = cand & ~twice
    bad = oversize | (cand & twice)
    ids = np.full(rows, NONE, np.int64)
    ids[bad] = INCONSISTENT
    roots = np.flatnonzero(good)              # ascending labels
    ids[roots] = np.arange(len(roots))
    track = np.where(root, ids, ids[label])
    track[size[label] < 2] = NONE
    members = np.flatnonzero(track >= 0)      # ascending rows; a stable sort by label keeps that
    out_rows = members[np.argsort(label[members], kind="stable")]
    offsets = np.concatenate([[0], np.cumsum(size[roots])]).astype(np.int64)
    stats = np.array([(n >= 2).sum(), len(roots), bad.sum(), short.sum()], np.int64)
    return Expected(track.astype(np.int32), offsets, out_rows.astype(np.int32), stats, len(roots))


# ---- the file format of tests/abi/tracks_check.cpp ----------------------------------------------

def write_cases(path, runs):
    """runs: [(Case, min_length)] in tracks_check's input format."""
    with open(path, "wb") as f:
        f.write(np.int32(len(runs)).tobytes())
        for case, ml in runs:
            counts = np.array([len(m) for m in case.matches], np.int32)
            f.write(np.array([len(case.offsets) - 1, len(case.pairs), ml], np.int32).tobytes())
            f.write(case.offsets.astype(np.int64).tobytes())
            f.write(case.pairs.astype(np.int32).tobytes())
            f.write(counts.tobytes())
            for m in case.matches:
                f.write(m.astype(np.int32).tobytes())


def read_results(path, n):
    raw = open(path, "rb").read()
    out, at = [], 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a
    for _ in range(n):
        T = int(take(np.int32, 1)[0])
        stats = take(np.int64, 4)
        rows = int(take(np.int32, 1)[0])
        track = take(np.int32, rows)
        offsets = take(np.int64, T + 1)
        out.append(Expected(track, offsets, take(np.int32, int(offsets[T])), stats, T))
    assert at == len(raw)
    return out


# ---- the cases ---------------------------------------------------------------------------------

def chain():
    """5 sets of 3 rows, a ring of pairs along row 1: one track of 5."""
    ring = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)]
    return _case([3] * 5, ring, [[(1, 1)]] * 5)


def reversed_repeated():
    """chain's edges given as (b, a); a pair listed twice and a pair without matches."""
    ring = [(1, 0), (2, 1), (3, 2), (4, 3), (0, 4), (2, 1), (3, 0)]
    return _case([3] * 5, ring, [[(1, 1)]] * 6 + [[]])


def fork(extra_sets: int):
    """0:0 - 1:0, 2:0 - 1:1 and 0:0 - 2:0: four rows, two of them in set 1.  Three sets: more rows
    than sets; with three more sets the ordering step has to find the two rows."""
    return _case([2] * (3 + extra_sets), [(0, 1), (2, 1), (0, 2)], [[(0, 0)], [(0, 1)], [(0, 0)]])


def self_pairs():
    """(a, a) with {i, i}: nothing; with {i, j}: two rows of one set."""
    return _case([4, 4, 4], [(1, 1), (2, 2), (0, 0)], [[(2, 2), (0, 0)], [(1, 3)], []])


LONG_CHAINS = [(0, 0, 130), (1, 0, 63), (1, 63, 64), (2, 0, 65), (3, 0, 127), (4, 0, 128), (5, 0, 129)]


def long_chains():
    """130 sets of 6 rows; chains along one row each, (row, first set, length) of LONG_CHAINS: the
    lengths on either side of the ordering kernel's 64-row step and of two steps, and one row of
    every set.  The pair list is shuffled."""
    rng = np.random.Generator(np.random.PCG64(4201))
    per_pair = collections.defaultdict(list)
    for row, first, length in LONG_CHAINS:
        for s in range(first, first + length - 1):
            per_pair[(s, s + 1)].append((row, row))
    pairs = list(per_pair)
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    return _case([6] * 130, pairs, [per_pair[p] for p in pairs])


def random_planted():
    """24 sets: sizes 0, 1, 37 and 21 of 200-400 rows.  Planted points, each seen in a random subset
    of the sets; all 276 pairs in shuffled order, each with about 70 % of its common points and 2 %
    wrong matches."""
    rng = np.random.Generator(np.random.PCG64(4202))
    nsets, npoints = 24, 1800
    small = {5: 0, 11: 1, 17: 37}
    big = [s for s in range(nsets) if s not in small]
    seen = [[] for _ in range(nsets)]
    for p in range(npoints):
        for s in rng.choice(big, rng.integers(1, 7), replace=False):
            seen[s].append(p)
    for s, n in small.items():
        seen[s] = list(rng.choice(npoints, n, replace=False))
    row_of = []
    for s in range(nsets):
        pts = rng.permutation(np.array(seen[s], np.int64))
        row_of.append({int(p): i for i, p in enumerate(pts)})
    sizes = [len(r) for r in row_of]
    assert all(200 <= sizes[s] <= 400 for s in big), sizes
    pairs = [(a, b) for a in range(nsets) for b in range(a + 1, nsets)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    matches = []
    for a, b in pairs:
        common = [p for p in row_of[a] if p in row_of[b]]
        m = [(row_of[a][p], row_of[b][p]) for p in common if rng.random() < 0.7]
        for _ in range(rng.binomial(len(common), 0.02) if sizes[a] and sizes[b] else 0):
            m.append((int(rng.integers(sizes[a])), int(rng.integers(sizes[b]))))
        matches.append(m)
    assert len(pairs) == 276
    return _case(sizes, pairs, matches)


def contended():
    """8 sets of 4096 rows, all 56 ordered pairs, identity matches: 229,376 edges, 4096 tracks of
    8, and many work items that unite the same components at once."""
    ident = np.stack([np.arange(4096), np.arange(4096)], axis=1).astype(np.int32)
    pairs = [(a, b) for a in range(8) for b in range(8) if a != b]
    return _case([4096] * 8, pairs, [ident] * len(pairs))


def empties():
    return {
        "empty no pairs": _case([3, 0, 5], [], []),
        "empty zero counts": _case([3, 0, 5], [(0, 2), (2, 0), (1, 1)], [[], [], []]),
        "empty sets": _case([0, 0, 0], [(0, 1), (2, 2)], [[], []]),
        "empty no sets": _case([], [], []),
    }


@functools.lru_cache(maxsize=None)
def cases():
    out = {
        "chain": chain(),
        "reversed repeated": reversed_repeated(),
        "fork 3 sets": fork(0),
        "fork 6 sets": fork(3),
        "self": self_pairs(),
        "long": long_chains(),
        "random": random_planted(),
        "contended": contended(),
    }
    out.update(empties())
    return out


NAMES = ["chain", "reversed repeated", "fork 3 sets", "fork 6 sets", "self", "long", "random",
         "contended", "empty no pairs", "empty zero counts", "empty sets", "empty no sets"]


@functools.lru_cache(maxsize=None)
def expected(name: str, min_length: int) -> Expected:
    e = numpy_tracks(cases()[name], min_length)
    for a in e[:4]:
        a.setflags(write=False)
    return e


def check_cases_do_their_job():
    """What the cases are there for, asserted on their own expected output."""
    for ml in MIN_LENGTHS:
        e = expected("chain", ml)
        assert e.T == 1 and e.rows.tolist() == [1, 4, 7, 10, 13] and e.stats.tolist() == [1, 1, 0, 0]
        r = expected("reversed repeated", ml)
        assert np.array_equal(r.track, e.track) and np.array_equal(r.rows, e.rows)
        for name in ("fork 3 sets", "fork 6 sets"):
            f = expected(name, ml)
            assert f.T == 0 and f.stats.tolist() == [1, 0, 1, 0]
            assert (f.track[[0, 2, 3, 4]] == INCONSISTENT).all() and (f.track == NONE).sum() == len(f.track) - 4
        lg = expected("long", ml)
        assert lg.T == len(LONG_CHAINS) and (lg.track >= 0).sum() == sum(n for _, _, n in LONG_CHAINS)
        assert sorted(np.diff(lg.offsets).tolist()) == sorted(n for _, _, n in LONG_CHAINS)
        c = expected("contended", ml)
        assert c.T == 4096 and (np.diff(c.offsets) == 8).all() and c.stats.tolist() == [4096, 4096, 0, 0]
        assert np.array_equal(c.track, np.tile(np.arange(4096), 8))
        for name in empties():
            z = expected(name, ml)
            assert z.T == 0 and (z.track == NONE).all() and z.offsets.tolist() == [0] and not z.stats.any()
    assert expected("self", 2).track.tolist() == [-1] * 8 + [-1, -2, -1, -2]
    assert expected("self", 2).stats.tolist() == [1, 0, 1, 0]
    assert expected("self", 3).stats.tolist() == [1, 0, 0, 1] and (expected("self", 3).track == NONE).all()
    assert (fork(0).offsets[-1], fork(3).offsets[-1]) == (6, 12)
    rnd2, rnd3 = expected("random", 2), expected("random", 3)
    assert rnd3.stats[1] > 100 and rnd3.stats[2] > 10 and rnd3.stats[3] > 10, rnd3.stats
    assert rnd2.stats[1] > rnd3.stats[1] and rnd2.stats[3] == 0 and (rnd2.track == NONE).any()
    assert np.diff(rnd3.offsets).max() <= 24 and np.diff(rnd3.offsets).min() >= 3
