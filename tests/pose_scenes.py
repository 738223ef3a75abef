"""Scenes, the host reference and a NumPy reference shared by the pose tests (test_pose.py on the
CPU, test_gpu_pose.py on the device, pose_time.py): two pinhole views with different intrinsics of
points under a planted motion, the edge pairs around them, a driver of tests/abi/pose_check.cpp --
the stand-alone program that runs spose::pose_host (csrc/sift_pose.h) on a pair list written with
numpy.tofile -- and numpy_pose, a float64 restatement of the rule that shares no code with it
(np.linalg.svd of K2' F K1, the four textbook decompositions, the same midpoint formula)."""
import collections
import functools
import os
import re
import subprocess
import tempfile

import numpy as np

import geom_scenes as G

KA = (500.0, 520.0, 320.0, 240.0)   # fx, fy, cx, cy of the first view
KB = (610.0, 600.0, 300.0, 260.0)   # and of the second: a swapped or transposed K cannot pass
THRESHOLD = 4.0
MIN_ANGLE = float(np.deg2rad(5.0))  # the planted scene's angles run from 2.9 to 8.1 degrees
PARALLEL_EPS = 1e-12                # csrc/sift_pose.h kParallelEps (test_pose.py compares them)
SIGMA_RATIO_MIN = 1e-3              # kSigmaRatioMin


def _rot(ay, ax):
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    return Ry @ Rx


R0 = _rot(0.08, -0.03)
T0 = np.array([0.6, 0.05, 0.1])


def kmat(k):
    return np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]])


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


def fundamental(R, t, ka, kb):
    """F of x_cam2 = R x_cam1 + t between cameras ka, kb, float64 at unit Frobenius norm, rounded
    to float32."""
    F = np.linalg.inv(kmat(kb)).T @ skew(t) @ R @ np.linalg.inv(kmat(ka))
    return (F / np.linalg.norm(F)).astype(np.float32)


F0 = fundamental(R0, T0, KA, KB)

Scene = collections.namedtuple("Scene", "la lb matches planted X")


@functools.lru_cache(maxsize=None)
def scene(seed=303, n=129, n_planted=129, noise=0.0):
    """n matches between the two views: n_planted of them are points at depth 4-8 seen under
    (R0, T0), with +-noise px of uniform noise in both views, the rest uniform random; coordinates
    rounded to float32, set b's rows permuted.  X [n][3]: the planted points in the first camera's
    frame (float64, from the coordinates before noise and rounding)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x1 = rng.uniform([0, 0], [640, 480], (n, 2))
    X = (np.c_[x1, np.ones(n)] @ np.linalg.inv(kmat(KA)).T) * rng.uniform(4, 8, (n, 1))
    c = (X @ R0.T + T0) @ kmat(KB).T
    x2 = c[:, :2] / c[:, 2:]
    if noise:
        x1 = x1 + rng.uniform(-noise, noise, (n, 2))
        x2 = x2 + rng.uniform(-noise, noise, (n, 2))
    planted = np.arange(n) < n_planted
    x2[~planted] = rng.uniform([0, 0], [640, 480], (n - n_planted, 2))
    order = rng.permutation(n)
    x1, x2, planted, X = x1[order], x2[order], planted[order], X[order]
    perm = rng.permutation(n)            # set b row perm[k] holds x2[k]
    lb = np.zeros_like(x2)
    lb[perm] = x2
    matches = np.stack([np.arange(n), perm], 1).astype(np.int32)
    return Scene(x1.astype(np.float32), lb.astype(np.float32), matches, planted, X)


def noisy_scene():
    """+-0.3 px of noise and 30 % random matches."""
    return scene(seed=404, n=400, n_planted=280, noise=0.3)


# ---- the host reference: spose::pose_host through tests/abi/pose_check.cpp -------------------------

@functools.lru_cache(maxsize=None)
def check_program(sanitize: bool) -> str:
    """pose_check built with g++, no contraction; under ASan + UBSan, or plain at -O2."""
    exe = os.path.join(tempfile.mkdtemp(prefix="pose_check_"), "pose_check")
    flags = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
             if sanitize else ["-O2"])
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags +
                       ["-I", G.CSRC, os.path.join(G.ROOT, "tests", "abi", "pose_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def header_constants():
    """{'sweeps': kPoseSweeps, 'ratio': kSigmaRatioMin, 'eps': kParallelEps} as the header has them."""
    out = subprocess.run([check_program(False), "info"], capture_output=True, text=True, check=True).stdout.split()
    return {out[0]: int(out[1]), out[2]: float(out[3]), out[4]: float(out[5])}


def write_list(d, loc, off, K, pairs, matches, F, threshold, min_angle):
    np.array([threshold, min_angle], np.float32).tofile(os.path.join(d, "params.bin"))
    np.ascontiguousarray(loc, np.float32).tofile(os.path.join(d, "loc.bin"))
    np.ascontiguousarray(off, np.int64).tofile(os.path.join(d, "offsets.bin"))
    np.ascontiguousarray(K, np.float32).reshape(-1, 4).tofile(os.path.join(d, "intrinsics.bin"))
    np.ascontiguousarray(pairs, np.int32).reshape(-1, 2).tofile(os.path.join(d, "pairs.bin"))
    ms = [np.ascontiguousarray(m, np.int32).reshape(-1, 2) for m in matches]
    np.concatenate(ms + [np.zeros((0, 2), np.int32)]).astype(np.int32).tofile(os.path.join(d, "matches.bin"))
    np.array([len(m) for m in ms], np.int32).tofile(os.path.join(d, "counts.bin"))
    np.ascontiguousarray(F, np.float32).reshape(-1, 9).tofile(os.path.join(d, "F.bin"))
    return [len(m) for m in ms]


HostPose = collections.namedtuple("HostPose", "R t participants front wide masks points candidates sweeps")


def host_pose(loc, off, K, pairs, matches, F, threshold=THRESHOLD, min_angle=MIN_ANGLE,
              sanitize=False, reps=1, times=None):
    """spose::pose_host on one pair list, in the layout SiftContext.pose_batch returns, and:
    candidates [npairs][4] = every candidate's in-front count, sweeps = the Jacobi sweeps the list's
    E needed.  times (a list) receives the host milliseconds of every repeat."""
    with tempfile.TemporaryDirectory(prefix="pose_scene_") as d:
        counts = write_list(d, loc, off, K, pairs, matches, F, threshold, min_angle)
        r = subprocess.run([check_program(sanitize), "run", d, str(reps)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        n = len(counts)
        R = np.fromfile(os.path.join(d, "R.bin"), np.float32).reshape(n, 3, 3)
        t = np.fromfile(os.path.join(d, "t.bin"), np.float32).reshape(n, 3)
        oc = np.fromfile(os.path.join(d, "out_counts.bin"), np.int32).reshape(n, 3)
        mask = np.fromfile(os.path.join(d, "mask.bin"), np.uint8)
        pts = np.fromfile(os.path.join(d, "points.bin"), np.float32).reshape(-1, 3)
        cand = np.fromfile(os.path.join(d, "front.bin"), np.int32).reshape(n, 4)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    assert len(mask) == offs[-1] == len(pts) and set(np.unique(mask)) <= {0, 1}
    if times is not None:
        times += [float(v) for v in re.findall(r"^host_ms ([0-9.]+)$", r.stdout, re.M)]
    sweeps = int(re.search(r"^sweeps_max (\d+)$", r.stdout, re.M).group(1))
    masks = [mask[offs[p]:offs[p + 1]].astype(bool) for p in range(n)]
    points = [pts[offs[p]:offs[p + 1]].copy() for p in range(n)]
    return HostPose(R, t, oc[:, 0].copy(), oc[:, 1].copy(), oc[:, 2].copy(), masks, points, cand, sweeps)


# ---- the pair lists -----------------------------------------------------------------------------------

FRONT = 5   # buffer rows in front of the first set
NAN_F = F0.copy()
NAN_F[1, 1] = np.nan
RANK1_F = np.outer(np.array([0.3, -0.5, 0.8], np.float32), np.array([1e-3, 2e-3, 0.9], np.float32)).astype(np.float32)
# a pure translation between two cameras KA: rays of one pixel in both views are parallel
SIDE_T = np.array([1.0, 0.2, 0.1])
PARALLEL_F = fundamental(np.eye(3), SIDE_T, KA, KA)

PairList = collections.namedtuple("PairList", "loc off K pairs matches F")


@functools.lru_cache(maxsize=None)
def pair_list():
    """The planted scene and the edge pairs around it, one call's worth.  Sets: 0, 1 = the scene's
    views (set 0 starts at buffer row FRONT), 2 = ten rows at one point (camera KA), 3 = empty.
    Pairs: 0 the scene; 1 an empty pair between real ones; 2 (b, a) under F0'; 3 the repeat;
    4 m = 0; 5 the identical points under a pure translation (parallel rays); 6 a zero F; 7 a
    rank-1 F; 8 an F with a NaN; 9 an empty set."""
    s = scene()
    same = np.tile(np.array([[100.5, 50.25]], np.float32), (10, 1))
    front = np.full((FRONT, 2), 7777.0, np.float32)
    loc = np.concatenate([front, s.la, s.lb, same])
    n = len(s.la)
    off = np.array([FRONT, FRONT + n, FRONT + 2 * n, len(loc), len(loc)], np.int64)
    K = np.array([KA, KB, KA, KB], np.float32)
    m = s.matches
    rev = m[:, ::-1][np.argsort(m[:, 1], kind="stable")]
    ident = np.stack([np.arange(10)] * 2, 1).astype(np.int32)
    none = np.zeros((0, 2), np.int32)
    pairs = [(0, 1), (0, 1), (1, 0), (0, 1), (0, 1), (2, 2), (0, 1), (0, 1), (0, 1), (3, 0)]
    matches = [m, none, rev, m, none, ident, m, m, m, none]
    F = np.stack([F0, F0, F0.T, F0, F0, PARALLEL_F, np.zeros((3, 3), np.float32), RANK1_F, NAN_F, F0])
    return PairList(loc, off, K, pairs, matches, np.ascontiguousarray(F, np.float32))


def rev_order():
    """Position k of pair 2's matches = position rev_order()[k] of pair 0's."""
    return np.argsort(scene().matches[:, 1], kind="stable")


LANE_COUNTS = (1, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def lane_list():
    """Pairs of m = 1, 63, 64, 65, 129 matches of the scene, in which the matches at positions
    0 and 63 (mod 64) -- the first and the last lane of a wave's stride -- are no participants: they
    point to a copy of their set-b row moved 40 px sideways, rows appended to set 1."""
    s = scene()
    n = len(s.la)
    moved = s.lb + np.array([3.0, 40.0], np.float32)
    loc = np.concatenate([s.la, s.lb, moved])
    off = np.array([0, n, 3 * n], np.int64)
    K = np.array([KA, KB], np.float32)
    matches = []
    for m in LANE_COUNTS:
        mt = s.matches[:m].copy()
        edge = np.isin(np.arange(m) % 64, (0, 63))
        mt[edge, 1] += n
        matches.append(mt)
    pairs = [(0, 1)] * len(LANE_COUNTS)
    F = np.stack([F0] * len(LANE_COUNTS))
    return PairList(loc, off, K, pairs, matches, F)


REAL = (0, 1023, 1024, 1025, 3004)


@functools.lru_cache(maxsize=None)
def filler_list():
    """3,000 eight-match filler pairs with the scene at positions REAL."""
    pl = pair_list()
    fill = pl.matches[0][:8]
    pairs = [(0, 1)] * 3005
    matches = [pl.matches[0] if p in REAL else fill for p in range(3005)]
    return PairList(pl.loc, pl.off, pl.K, pairs, matches, np.stack([F0] * 3005))


# ---- the NumPy reference -----------------------------------------------------------------------------

W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])

RefPose = collections.namedtuple(
    "RefPose", "ok R t part part_clear candidates best l1 l2 det angle front clear X")


def numpy_pose(F, ka, kb, x1, x2, threshold=THRESHOLD, min_angle=MIN_ANGLE):
    """The rule in float64 for one pair.  candidates [4]: the in-front participants of the four
    textbook decompositions (R1, +u3), (R1, -u3), (R2, +u3), (R2, -u3) of np.linalg.svd -- their
    order is the SVD's, not the library's; best = the first with the most.  Under the best: depths
    l1, l2, determinant, angle (rad) and point X of every match; front = in front; clear = l1, l2
    and the determinant are clear of their limits by 1e-9 relative and the angle of min_angle by
    1e-6 rad; part_clear = the Sampson error is clear of the threshold by 1e-3 relative."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    x1 = np.asarray(x1, np.float64)
    x2 = np.asarray(x2, np.float64)
    err = G.predicate64("F", F, x1, x2)
    with np.errstate(invalid="ignore"):
        part = err < threshold
        part_clear = ~(np.abs(err - threshold) <= 1e-3 * threshold)
    E = kmat(kb).T @ F @ kmat(ka)
    nrm = np.linalg.norm(E)
    none = RefPose(False, np.zeros((3, 3)), np.zeros(3), part, part_clear, np.zeros(4, int), 0,
                   None, None, None, None, np.zeros(len(x1), bool), np.ones(len(x1), bool), None)
    if not (np.isfinite(nrm) and nrm > 0):
        return none
    U, S, Vt = np.linalg.svd(E / nrm)
    if not S[1] > SIGMA_RATIO_MIN * S[0]:
        return none
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    a = np.c_[x1, np.ones(len(x1))] @ np.linalg.inv(kmat(ka)).T
    b = np.c_[x2, np.ones(len(x2))] @ np.linalg.inv(kmat(kb)).T

    def triangulate(R, t):
        c = a @ R.T
        cc, bb, cb = (c * c).sum(1), (b * b).sum(1), (c * b).sum(1)
        det = (np.cross(c, b) ** 2).sum(1)
        ct, bt = c @ t, b @ t
        with np.errstate(all="ignore"):
            l1 = (cb * bt - bb * ct) / det
            l2 = (cc * bt - cb * ct) / det
            front = (det > PARALLEL_EPS) & (l1 > 0) & (l2 > 0)
            X = (l1[:, None] * a + (l2[:, None] * b - t) @ R) / 2
            angle = np.arccos(np.clip(cb / np.sqrt(cc * bb), -1, 1))
        return l1, l2, det, angle, front, X

    cands = [(U @ W @ Vt, U[:, 2]), (U @ W @ Vt, -U[:, 2]), (U @ W.T @ Vt, U[:, 2]), (U @ W.T @ Vt, -U[:, 2])]
    counts = np.array([int((triangulate(R, t)[4] & part).sum()) for R, t in cands])
    best = int(np.argmax(counts))
    R, t = cands[best]
    l1, l2, det, angle, front, X = triangulate(R, t)
    with np.errstate(invalid="ignore"):
        clear = ((np.abs(l1) > 1e-9 * np.maximum(1.0, np.abs(l1))) & (np.abs(l2) > 1e-9 * np.maximum(1.0, np.abs(l2)))
                 & (np.abs(det - PARALLEL_EPS) > 1e-9 * PARALLEL_EPS) & (np.abs(angle - min_angle) > 1e-6))
    clear |= det <= PARALLEL_EPS * (1 - 1e-9)   # parallel rays: whatever l1, l2 are
    return RefPose(True, R, t, part, part_clear, counts, best, l1, l2, det, angle, front, clear, X)


def pair_points(pl, p):
    """x1, x2 [m][2] float32 of pair p's matches."""
    a, b = pl.pairs[p]
    m = np.asarray(pl.matches[p]).reshape(-1, 2)
    return pl.loc[pl.off[a] + m[:, 0]], pl.loc[pl.off[b] + m[:, 1]]
