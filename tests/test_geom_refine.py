"""The local refinement of the geometry estimator (sgeo::refine_host, csrc/sift_geom.h), checked
without a GPU.

tests/abi/geom_refine_check.cpp includes only that header and is built with g++ -ffp-contract=off
under AddressSanitizer and UBSan.  Its self-checks: the cyclic Jacobi solver on a diagonal matrix
and on 1,000 random PSD 9 x 9 matrices (residual <= 1e-12 of the matrix norm, the smallest
diagonal entry wins, ties to the lowest index), exact H and F scenes refit within kSolveTol, points
at one location are an invalid refit, and the sweep count behind kJacobiSweeps.

In file mode the program runs sgeo::refine_host on the scenes of geom_scenes.pair_list().  Its
results are pinned by means that do not use the new code: the oracle's guided_pass for every mask
bit, a NumPy float64 SVD refit (normalised DLT / eight-point) of the unrefined inliers for the
model of one round, the planted matches for the gain at tight thresholds, and sgeo::estimate_host
(geom_check) for rounds = 0."""
import functools
import subprocess

import numpy as np
import pytest

import geom_refine_scenes as R
import geom_scenes as G
import oracle_py as O

EYE = np.eye(3, dtype=np.float32)
CASES = {"H": G.H_CASE, "F": G.F_CASE}
TIGHT = {"H": R.H_TIGHT, "F": R.F_TIGHT}
FITTED = (0, 2, 3, 7)   # pair positions with a model whose refit is compared


@functools.lru_cache(maxsize=None)
def _refined(model, rounds, tight=False):
    loc, off, pairs, matches, _ = G.pair_list(model)
    info = {}
    case = (TIGHT if tight else CASES)[model]
    out = R.host_refine(loc, off, pairs, matches, rounds=rounds, sanitize=True, info=info, **case)
    return out + (info,)


@functools.lru_cache(maxsize=None)
def _unrefined(model, tight=False):
    loc, off, pairs, matches, _ = G.pair_list(model)
    return G.host_estimate(loc, off, pairs, matches, **(TIGHT if tight else CASES)[model])


def _points(loc, off, pair, m):
    a, b = pair
    return loc[off[a] + m[:, 0]], loc[off[b] + m[:, 1]]


def test_refine_self_checks_under_sanitizers():
    r = subprocess.run([R.check_program(True)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refine ok" in r.stdout


def test_sweep_constant_is_the_measured_maximum_plus_two():
    """kJacobiSweeps = 2 + the most sweeps that any refit matrix of the test scenes (shipped and
    tight thresholds, unrefined and returned models) or any of the 1,000 random PSD matrices needs
    for an off-diagonal norm <= 1e-14 of its Frobenius norm."""
    out = subprocess.run([R.check_program(False)], capture_output=True, text=True, check=True).stdout
    worst = int(out.split("sweeps_random")[1].split()[0])
    for model in ("H", "F"):
        for tight in (False, True):
            worst = max(worst, _refined(model, 8, tight)[4]["sweeps"])
    assert R.header_constants() == {"sweeps": worst + 2, "lanes": 64}


@pytest.mark.parametrize("model", ["H", "F"])
def test_zero_rounds_are_the_unrefined_bytes(model):
    m0, i0, k0 = _unrefined(model)
    m, i, k, done, _ = _refined(model, 0)
    assert m.tobytes() == m0.tobytes() and i.tolist() == i0.tolist() and not done.any()
    assert all(np.array_equal(a, b) for a, b in zip(k, k0))


@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("model", ["H", "F"])
def test_masks_are_the_guided_test_of_the_returned_matrix(model, tight):
    thr = (TIGHT if tight else CASES)[model]["threshold"]
    loc, off, pairs, matches, _ = G.pair_list(model)
    for rounds in (1, 8):
        models, inliers, masks, done, _ = _refined(model, rounds, tight)
        assert done.max() >= 1 and done.max() <= rounds
        for p, (pair, m) in enumerate(zip(pairs, matches)):
            assert len(masks[p]) == len(m) and inliers[p] == masks[p].sum(), p
            x1, x2 = _points(loc, off, pair, m)
            H, F, hd, fd = (models[p], EYE, thr, 1e20) if model == "H" else (EYE, models[p], 1e20, thr)
            want = [O.guided_pass(H, F, float(a[0]), float(a[1]), float(b[0]), float(b[1]), hd, fd)
                    for a, b in zip(x1, x2)]
            assert masks[p].tolist() == want, p
            assert abs(float(np.linalg.norm(models[p])) - 1.0) < 1e-6 or not models[p].any()
            if not models[p].any():
                assert inliers[p] == 0 and done[p] == 0


def _normalise(x):
    """centroid to the origin, mean absolute deviation per coordinate to 1: (points, T)"""
    c = x.mean(0)
    s = 1.0 / np.abs(x - c).mean()
    T = np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]])
    return (x - c) * s, T


def _svd_refit(model, x1, x2):
    """least squares over the correspondences, NumPy float64: the normalised DLT / eight-point"""
    u1, T1 = _normalise(x1.astype(np.float64))
    u2, T2 = _normalise(x2.astype(np.float64))
    n, one, zero = len(u1), np.ones(len(u1)), np.zeros(len(u1))
    if model == "H":
        a = np.c_[zero, zero, zero, -u1[:, 0], -u1[:, 1], -one, u2[:, 1] * u1[:, 0], u2[:, 1] * u1[:, 1], u2[:, 1]]
        b = np.c_[u1[:, 0], u1[:, 1], one, zero, zero, zero, -u2[:, 0] * u1[:, 0], -u2[:, 0] * u1[:, 1], -u2[:, 0]]
        A = np.concatenate([a, b])
    else:
        A = np.c_[u2[:, 0] * u1[:, 0], u2[:, 0] * u1[:, 1], u2[:, 0], u2[:, 1] * u1[:, 0],
                  u2[:, 1] * u1[:, 1], u2[:, 1], u1[:, 0], u1[:, 1], one]
    g = np.linalg.svd(A)[2][-1].reshape(3, 3)
    M = np.linalg.inv(T2) @ g @ T1 if model == "H" else T2.T @ g @ T1
    assert n >= G.MIN_SAMPLE[model]
    return M / np.linalg.norm(M)


def _geometry(model, M, x1, x2):
    """H: the transferred points; F: the signed distance of x2 from the epipolar line F x1"""
    a = np.c_[x1.astype(np.float64), np.ones(len(x1))]
    if model == "H":
        h = a @ M.T
        return h[:, :2] / h[:, 2:]
    l = a @ M.T
    return (np.c_[x2.astype(np.float64), np.ones(len(x2))] * l).sum(1) / np.hypot(l[:, 0], l[:, 1])


@pytest.mark.parametrize("model", ["H", "F"])
def test_one_round_is_the_least_squares_refit_of_the_inliers(model):
    """rounds = 1 against an SVD refit in NumPy float64 of the unrefined mask's inliers, sign
    aligned: the geometry of those inliers differs by < 1e-3 px (float32 rounding of the model
    included), and the RMS of the predicate over them is strictly lower than before."""
    loc, off, pairs, matches, _ = G.pair_list(model)
    m0, _, k0 = _unrefined(model)
    m1, _, _, done, _ = _refined(model, 1)
    for p in FITTED:
        assert done[p] == 1 and k0[p].sum() >= G.MIN_SAMPLE[model], p
        x1, x2 = _points(loc, off, pairs[p], matches[p])
        x1, x2 = x1[k0[p]], x2[k0[p]]
        want = _svd_refit(model, x1, x2)
        got = m1[p].astype(np.float64)
        got = got / np.linalg.norm(got) * np.sign((got * want).sum())
        diff = float(np.abs(_geometry(model, got, x1, x2) - _geometry(model, want, x1, x2)).max())
        before = float(np.sqrt((G.predicate64(model, m0[p], x1, x2) ** 2).mean()))
        after = float(np.sqrt((G.predicate64(model, m1[p], x1, x2) ** 2).mean()))
        print(f"{model} position {p}: {int(k0[p].sum())} inliers, refit differs by {diff:.3g} px, "
              f"predicate RMS {before:.6g} -> {after:.6g}")
        assert diff < 1e-3, (p, diff)
        assert after < before, (p, before, after)


@pytest.mark.parametrize("model", ["H", "F"])
def test_tight_thresholds_gain_the_planted_inliers(model):
    """H at 0.45 px, F at 0.15 px^2, rounds = 8: the unrefined winner misses planted matches that
    the refit finds."""
    *_, planted = G.pair_list(model)
    _, i0, _ = _unrefined(model, True)
    _, i8, k8, done, _ = _refined(model, 8, True)
    n_planted = int(planted.sum())
    for p in (0, 2, 3):
        print(f"{model} position {p}: {i0[p]} -> {i8[p]} inliers in {done[p]} rounds ({n_planted} planted)")
        assert i8[p] - i0[p] >= (5 if model == "H" else 25), (p, i0[p], i8[p])
        assert i8[p] >= 0.95 * n_planted
    assert (k8[0] & planted).sum() >= 0.95 * n_planted


@pytest.mark.parametrize("model", ["H", "F"])
def test_inliers_never_decrease_with_the_round_budget(model):
    for tight in (False, True):
        prev = _unrefined(model, tight)[1]
        for rounds in range(9):
            _, inl, _, done, info = _refined(model, rounds, tight)
            assert (inl >= prev).all(), (tight, rounds, inl, prev)
            assert (done <= rounds).all()
            prev = inl


def test_a_round_that_loses_an_inlier_is_rejected():
    """F at 0.15 px^2: at positions 0 and 2 the third refit scores below the second and is dropped:
    the result of any larger budget is the result of two rounds."""
    two = _refined("F", 2, True)
    for rounds in (3, 8):
        more = _refined("F", rounds, True)
        for p in (0, 2):
            assert more[4]["stops"][p] == "rejected" and more[3][p] == 2
            assert more[0][p].tobytes() == two[0][p].tobytes() and more[1][p] == two[1][p]
    stops = _refined("F", 8, True)[4]["stops"]
    assert stops[1] == stops[4] == stops[5] == stops[8] == stops[9] == "no model"
    assert stops[3] == stops[6] == "fixed point"
    assert _refined("H", 1, True)[4]["stops"][0] == "budget"
