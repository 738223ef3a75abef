"""The geometry estimator's host side (csrc/sift_geom.h), checked without a GPU.

tests/abi/geom_check.cpp includes only that header and is built with g++ -ffp-contract=off under
AddressSanitizer and UBSan.  Its self-checks: samples are distinct and in range (m = 4, 5, 8, 9,
1000), H of four planted correspondences maps them back and F of eight annihilates them within the
header's kSolveTol (a sideways translation with F33 = 0 included), repeated and collinear samples
are invalid, the planner covers every (pair, block) once and gives pairs below the minimal sample
no items.

In file mode the program runs sgeo::estimate_host on the planted scenes and the edge pairs of
geom_scenes.pair_list().  Its results are checked against references that do not use the new code:
the oracle's guided_pass (the guided matcher's own test, other matrix disabled) for every mask
bit, a NumPy float64 restatement of the predicate away from the threshold, and the planted
matches for recovery: the mask must cover at least 95 % of them (an all-inlier sample has chance
0.6^4 = 0.13 for H and 0.7^8 = 0.058 for F, so missing over 512 / 1024 hypotheses is below
1e-25)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import geom_scenes as G
import oracle_py as O

EYE = np.eye(3, dtype=np.float32)


def test_geom_self_checks_under_sanitizers():
    r = subprocess.run([G.check_program(True)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "geom ok" in r.stdout


def test_geom_header_includes_no_hip():
    src = open(os.path.join(G.CSRC, "sift_geom.h")).read()
    assert "hip" not in "".join(l for l in src.splitlines(True) if l.lstrip().startswith("#include"))


@functools.lru_cache(maxsize=None)
def _host(model):
    case = G.H_CASE if model == "H" else G.F_CASE
    loc, off, pairs, matches, planted = G.pair_list(model)
    return G.host_estimate(loc, off, pairs, matches, sanitize=True, **case)


def _points(loc, off, pair, m):
    a, b = pair
    return loc[off[a] + m[:, 0]], loc[off[b] + m[:, 1]]


@pytest.mark.parametrize("model", ["H", "F"])
def test_masks_are_the_guided_test(model):
    case = G.H_CASE if model == "H" else G.F_CASE
    thr = case["threshold"]
    loc, off, pairs, matches, _ = G.pair_list(model)
    models, inliers, masks = _host(model)
    checked = 0
    for p, (pair, m) in enumerate(zip(pairs, matches)):
        assert len(masks[p]) == len(m) and inliers[p] == masks[p].sum(), p
        x1, x2 = _points(loc, off, pair, m)
        H, F, hd, fd = (models[p], EYE, thr, 1e20) if model == "H" else (EYE, models[p], 1e20, thr)
        want = [O.guided_pass(H, F, float(a[0]), float(a[1]), float(b[0]), float(b[1]), hd, fd)
                for a, b in zip(x1, x2)]
        assert masks[p].tolist() == want, p
        if len(m) and models[p].any():
            err = G.predicate64(model, models[p], x1, x2)
            clear = np.abs(err - thr) > 1e-3 * thr
            assert clear.sum() >= 0.9 * len(m)
            assert np.array_equal(masks[p][clear], (err < thr)[clear]), p
            checked += int(clear.sum())
        assert abs(float(np.linalg.norm(models[p])) - 1.0) < 1e-6 or not models[p].any()
    assert checked > 2 * len(matches[0])


@pytest.mark.parametrize("model", ["H", "F"])
def test_planted_recovery_and_edge_pairs(model):
    S = G.MIN_SAMPLE[model]
    loc, off, pairs, matches, planted = G.pair_list(model)
    models, inliers, masks = _host(model)
    n_planted = int(planted.sum())
    assert n_planted == (180 if model == "H" else 280)
    # the scene (twice: another pair position draws other samples) and its (b, a) form
    rev_planted = planted[np.argsort(matches[0][:, 1], kind="stable")]
    for p, pl in ((0, planted), (3, planted), (2, rev_planted)):
        assert (masks[p] & pl).sum() >= 0.95 * n_planted, (p, int((masks[p] & pl).sum()))
        assert inliers[p] < 1.15 * n_planted   # and not everything
    assert not np.array_equal(models[0], models[3])
    # no model: zeros, 0 inliers, zero mask
    for p in (1, 4, 5, 8, 9):
        assert len(matches[p]) in (0, S - 1, S + 2)
        assert not models[p].any() and inliers[p] == 0 and not masks[p].any(), p
    # m = S: the one sample, every hypothesis the same set; its matches are exact inliers of it
    assert [len(matches[p]) for p in (6, 7)] == [S, S + 1]
    assert inliers[6] == S and inliers[7] >= S
