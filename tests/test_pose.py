"""The pose rule's host side (csrc/sift_pose.h), checked without a GPU.

tests/abi/pose_check.cpp includes only that header and is built with g++ -ffp-contract=off under
AddressSanitizer and UBSan.  Its self-checks: a planted motion between two different cameras is
exactly one of the four candidates, every candidate is a rotation, a point in front of both cameras
is in front under that candidate alone and triangulates to itself; a zero, rank-1, NaN or infinite
F has no pose; the argument checks.  It also measures the Jacobi sweeps that 1,000 random E need.

In file mode the program runs spose::pose_host on the pair lists of pose_scenes.  Its results are
held to pose_scenes.numpy_pose, a float64 restatement that shares no code with the header
(np.linalg.svd of K2' F K1, the four textbook decompositions, the same midpoint formula), and to
the planted motion.

Bounds.  The yardstick is the NumPy reference's own deviation from the planted values on the
noise-free scene, where the only errors are the float32 rounding of the coordinates and of F.
Measured on an x86-64 host: |R - R0| <= 4.3e-9, |t - t0 / |t0|| <= 2.8e-9, points
after rescaling by |t0| within 8.7e-6.  pose_host is held to 16 times each (the margin is there for
the squared conditioning of E'E and the float32 rounding of the outputs): 6.8e-8, 4.5e-8, 1.4e-4.
The tests take the deviations from the reference at run time, so the bound follows the reference on
another LAPACK, and assert that they have not left the order of magnitude written here.  pose_host
itself gave 3.0e-8, 5.3e-9 and 8.9e-6."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import geom_refine_scenes as GR
import geom_scenes as G
import pose_scenes as S
import sgpu

ROOT = G.ROOT
T0N = S.T0 / np.linalg.norm(S.T0)
MARGIN = 16


@functools.lru_cache(maxsize=None)
def _self_checks():
    r = subprocess.run([S.check_program(True)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@functools.lru_cache(maxsize=None)
def _host(threshold=S.THRESHOLD):
    return S.host_pose(*S.pair_list(), threshold=threshold, sanitize=True)


@functools.lru_cache(maxsize=None)
def _reference():
    """The NumPy reference on the planted scene and its deviations from the planted values:
    (reference, |R - R0|, |t - t0 / |t0||, point error after rescaling)."""
    pl = S.pair_list()
    x1, x2 = S.pair_points(pl, 0)
    r = S.numpy_pose(pl.F[0], S.KA, S.KB, x1, x2)
    assert r.ok and r.front.all()
    dev_R = float(np.abs(r.R - S.R0).max())
    dev_t = float(np.abs(r.t - T0N).max())
    dev_X = float(np.abs(r.X * np.linalg.norm(S.T0) - S.scene().X).max())
    print(f"reference deviations: R {dev_R:.3g} t {dev_t:.3g} points {dev_X:.3g}")
    # the figures of the module docstring, within a factor of four either way
    assert 4.3e-9 / 4 < dev_R < 4.3e-9 * 4 and 2.8e-9 / 4 < dev_t < 2.8e-9 * 4
    assert 8.7e-6 / 4 < dev_X < 8.7e-6 * 4
    return r, dev_R, dev_t, dev_X


@functools.lru_cache(maxsize=None)
def _noisy():
    """The noisy scene as one pair, its F by sgeo::estimate_host and three rounds of refinement
    (the geom_check / geom_refine_check programs), and pose_host on it."""
    s = S.noisy_scene()
    n = len(s.la)
    loc = np.concatenate([s.la, s.lb])
    off = np.array([0, n, 2 * n], np.int64)
    models, inliers, _ = G.host_estimate(loc, off, [(0, 1)], [s.matches], **G.F_CASE)
    assert inliers[0] >= 0.9 * s.planted.sum()
    refined, inliers2, _, _ = GR.host_refine(loc, off, [(0, 1)], [s.matches], rounds=3, **G.F_CASE)
    assert inliers2[0] >= inliers[0]
    pl = S.PairList(loc, off, np.array([S.KA, S.KB], np.float32), [(0, 1)], [s.matches], refined)
    return pl, S.host_pose(*pl, sanitize=True)


def _same_decisions(host, p, ref):
    """Mask and wide count of pair p against the reference, wherever the reference is clear of its
    limits; at most 2 % of the matches may be left out.  Returns how many were."""
    use = ref.clear & ref.part_clear
    out = int((~use).sum())
    assert out <= 0.02 * len(use), out
    want = ref.part & ref.front
    assert np.array_equal(host.masks[p][use], want[use])
    assert host.participants[p] - out <= int(ref.part.sum()) <= host.participants[p] + out
    wide = want & (ref.angle >= S.MIN_ANGLE)
    assert abs(int(host.wide[p]) - int(wide.sum())) <= out
    assert abs(int(host.front[p]) - int(want.sum())) <= out
    return out


def test_pose_self_checks_under_sanitizers():
    assert "pose ok" in _self_checks()


def test_pose_header_includes_no_hip():
    src = open(os.path.join(G.CSRC, "sift_pose.h")).read()
    includes = [l for l in src.splitlines() if l.lstrip().startswith("#include")]
    assert includes == ['#include "sift_geom.h"']
    assert "namespace spose" in src and "inline void pose_host" in src


def test_sweep_count_is_the_measured_maximum_plus_two():
    random_max = int(re.search(r"^sweeps_max (\d+)$", _self_checks(), re.M).group(1))
    scenes_max = max(_host().sweeps, _noisy()[1].sweeps)
    print(f"sweeps: random E {random_max}, scenes {scenes_max}")
    assert max(random_max, scenes_max) + 2 == S.header_constants()["sweeps"]


def test_header_constants_are_the_reference_ones():
    c = S.header_constants()
    assert c["eps"] == S.PARALLEL_EPS and c["ratio"] == S.SIGMA_RATIO_MIN


def test_planted_scene_against_numpy_and_the_planted_pose():
    ref, dev_R, dev_t, dev_X = _reference()
    h = _host()
    assert h.candidates[0].tolist() == [0, 129, 0, 0]
    assert sorted(ref.candidates.tolist()) == [0, 0, 0, 129]
    assert np.abs(h.R[0] - ref.R).max() <= MARGIN * dev_R
    assert np.abs(h.t[0] - ref.t).max() <= MARGIN * dev_t
    assert np.abs(h.R[0] - S.R0).max() <= MARGIN * dev_R
    assert np.abs(h.t[0] - T0N).max() <= MARGIN * dev_t
    assert abs(np.linalg.det(h.R[0].astype(np.float64)) - 1) < 1e-6
    assert _same_decisions(h, 0, ref) == 0          # the reference excludes none here
    assert (h.participants[0], h.front[0]) == (129, 129) and h.masks[0].all()
    # 5 degrees splits the matches
    assert 0 < h.wide[0] < 129 and h.wide[0] == int((ref.angle >= S.MIN_ANGLE).sum())
    assert np.degrees(ref.angle.min()) > 2 and np.degrees(ref.angle.max()) < 9
    got = h.points[0].astype(np.float64) * np.linalg.norm(S.T0)
    assert np.abs(got - S.scene().X).max() <= MARGIN * dev_X
    assert np.abs(h.points[0] - ref.X).max() * np.linalg.norm(S.T0) <= MARGIN * dev_X


def test_noisy_scene_against_numpy_and_the_planted_matches():
    _, dev_R, dev_t, _ = _reference()
    pl, h = _noisy()
    s = S.noisy_scene()
    x1, x2 = S.pair_points(pl, 0)
    ref = S.numpy_pose(pl.F[0], S.KA, S.KB, x1, x2)
    assert ref.ok
    assert np.abs(h.R[0] - ref.R).max() <= MARGIN * dev_R
    assert np.abs(h.t[0] - ref.t).max() <= MARGIN * dev_t
    assert sorted(h.candidates[0].tolist()) == sorted(ref.candidates.tolist())
    _same_decisions(h, 0, ref)
    n_planted = int(s.planted.sum())
    assert int((h.masks[0] & s.planted).sum()) >= 0.95 * n_planted
    w = int(np.argmax(h.candidates[0]))
    assert h.candidates[0][w] == h.front[0]
    assert all(c <= 0.05 * n_planted for k, c in enumerate(h.candidates[0]) if k != w)
    # the pose is the planted one as far as 0.3 px of noise allow
    assert np.abs(h.R[0] - S.R0).max() < 0.02 and np.abs(h.t[0] - T0N).max() < 0.1


def test_edge_pairs():
    _, dev_R, dev_t, _ = _reference()
    pl = S.pair_list()
    h = _host()
    assert pl.off[0] == S.FRONT == 5
    assert [len(m) for m in pl.matches] == [129, 0, 129, 129, 0, 10, 129, 129, 129, 0]
    # (b, a) under F' gives (R', -R't), match by match
    R, t = h.R[0].astype(np.float64), h.t[0].astype(np.float64)
    assert np.abs(h.R[2] - R.T).max() <= MARGIN * dev_R
    assert np.abs(h.t[2] + R.T @ t).max() <= MARGIN * dev_t
    order = S.rev_order()
    assert (h.participants[2], h.front[2], h.wide[2]) == (h.participants[0], h.front[0], h.wide[0])
    assert np.array_equal(h.masks[2], h.masks[0][order])
    # its points are the same points in the second camera's frame
    X2 = h.points[0][order].astype(np.float64) @ R.T + t
    assert np.abs(h.points[2] - X2).max() < 1e-4
    # the repeat gives the same bytes
    for a in ("R", "t", "points"):
        assert getattr(h, a)[3].tobytes() == getattr(h, a)[0].tobytes(), a
    assert np.array_equal(h.masks[3], h.masks[0]) and h.wide[3] == h.wide[0]
    # no result: m = 0, an empty set, parallel rays, no pose
    for p in (1, 4, 9):
        assert (h.participants[p], h.front[p], h.wide[p]) == (0, 0, 0) and not h.R[p].any()
    assert (h.participants[5], h.front[5], h.wide[5]) == (10, 0, 0)
    for p in (5, 6, 7, 8):
        assert h.front[p] == 0 and h.wide[p] == 0 and not h.candidates[p].any(), p
        assert not h.R[p].any() and not h.t[p].any() and not h.masks[p].any() and not h.points[p].any(), p
    assert h.participants[6] == 0 and h.participants[8] == 0     # a zero or NaN F passes nothing
    # the reference agrees that these have no pose (5: a pose, but nothing in front)
    for p in (6, 7, 8):
        assert not S.numpy_pose(pl.F[p], S.KA, S.KB, *S.pair_points(pl, p)).ok, p
    r5 = S.numpy_pose(pl.F[5], S.KA, S.KA, *S.pair_points(pl, 5))
    assert r5.ok and r5.part.all() and not r5.candidates.any()


def test_threshold_1e20_takes_every_match():
    pl = S.pair_list()
    h = _host(1e20)
    # every match of a pair whose F is finite and not zero
    for p in (0, 2, 3, 5, 7):
        assert h.participants[p] == len(pl.matches[p]), p
    assert h.participants[6] == 0 and h.participants[8] == 0
    assert h.front.tolist() == _host().front.tolist()
    # the displaced matches of the lane list participate now, and still lie in front or not
    ll = S.lane_list()
    tight, loose = S.host_pose(*ll), S.host_pose(*ll, threshold=1e20)
    for p, m in enumerate(S.LANE_COUNTS):
        edge = np.isin(np.arange(m) % 64, (0, 63))
        assert tight.participants[p] == m - edge.sum() and loose.participants[p] == m
        assert not tight.masks[p][edge].any() and tight.masks[p][~edge].all()
        assert tight.front[p] == m - edge.sum()


def test_header_is_plain_c_and_declares_pose(tmp_path):
    src = os.path.join(ROOT, "tests", "abi", "pose_abi.c")
    obj = str(tmp_path / "pose_abi.o")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I",
                        os.path.join(ROOT, "include"), "-c", "-o", obj, src],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    syms = subprocess.check_output(["nm", obj], text=True)
    for name in ("sgpu_pose_batch", "sgpu_pose_images"):
        assert f" U {name}" in syms, name


def test_null_context_needs_no_device():
    L = sgpu.lib()
    loc = (ctypes.c_float * 8)()
    off = (ctypes.c_int64 * 3)(0, 2, 4)
    K = (ctypes.c_float * 8)(500, 500, 320, 240, 500, 500, 320, 240)
    pairs = (ctypes.c_int * 2)(0, 1)
    matches = (ctypes.c_int * 2)(1, 1)
    counts = (ctypes.c_int * 1)(1)
    F = (ctypes.c_float * 9)(0, 0, 0, 0, 0, -1, 0, 1, 0)
    R = (ctypes.c_float * 9)(*[7] * 9)
    t = (ctypes.c_float * 3)(7, 7, 7)
    oc = (ctypes.c_int * 3)(7, 7, 7)
    mask = (ctypes.c_uint8 * 1)(7)
    pts = (ctypes.c_float * 3)(7, 7, 7)
    assert L.sgpu_pose_batch(None, loc, off, 2, K, pairs, 1, matches, counts, F, 4.0, 0.05, R, t, oc,
                             mask, pts, sgpu.SGPU_INPUT_HOST) == sgpu.SGPU_EINVAL
    assert L.sgpu_pose_images(None, K, pairs, 1, matches, counts, F, 4.0, 0.05, R, t, oc, mask,
                              pts) == sgpu.SGPU_EINVAL
    assert list(R) + list(t) + list(oc) + list(mask) + list(pts) == [7] * 19


def test_binding_rejects_wrong_shapes():
    """The binding's ValueErrors come before any C call: no device needed."""
    ctx = sgpu.SiftContext.__new__(sgpu.SiftContext)
    ctx._ctx = None
    ctx.batch = 2
    loc = np.zeros((10, 2), np.float32)
    off = [0, 4, 10]
    m = np.zeros((3, 2), np.int32)
    F = np.zeros((1, 3, 3), np.float32)
    K = np.array([S.KA, S.KB], np.float32)
    bad = [dict(loc=np.zeros((10, 4), np.float32)), dict(offsets=[0, 4, 11]), dict(pairs=[(0, 1, 1)]),
           dict(matches=[m, m]), dict(matches=[np.zeros((2, 3), np.int32)]),
           dict(F=np.zeros((2, 3, 3), np.float32)), dict(F=np.zeros((3, 3, 1), np.float32)),
           dict(K=K[:1]), dict(K=np.zeros((2, 3), np.float32)), dict(threshold=-1.0),
           dict(threshold=float("nan")), dict(min_angle=-0.1), dict(min_angle=1.6)]
    good = dict(loc=loc, offsets=off, pairs=[(0, 1)], matches=[m], F=F, K=K)
    for b in bad:
        with pytest.raises(ValueError):
            ctx.pose_batch(**dict(good, **b))
    for b in (dict(matches=[]), dict(F=F[0, 0]), dict(K=np.zeros((3, 4), np.float32)), dict(min_angle=2.0)):
        with pytest.raises(ValueError):
            ctx.pose_images(**dict(dict(pairs=[(0, 1)], matches=[m], F=F, K=K), **b))
    assert sgpu.Pose._fields == ("R", "t", "participants", "front", "wide", "masks", "points")
