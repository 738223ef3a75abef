"""Scenes and the host reference shared by the geometry estimator's tests (test_geom.py on the CPU,
test_gpu_estimate.py on the device): planted H and F scenes, the edge pairs around them, and a
driver of tests/abi/geom_check.cpp, the stand-alone program that runs sgeo::estimate_host
(csrc/sift_geom.h) on a scene written with numpy.tofile."""
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modify-sift-gpu_amd", "csrc")
MODELS = {"H": 0, "F": 1}
MIN_SAMPLE = {"H": 4, "F": 8}
# (threshold, iterations, scene seed, estimator seed) of the two planted scenes
H_CASE = dict(model="H", threshold=2.0, iterations=512, seed=11)
F_CASE = dict(model="F", threshold=4.0, iterations=1024, seed=12)


@functools.lru_cache(maxsize=None)
def check_program(sanitize: bool) -> str:
    """geom_check built with g++, no contraction; under ASan + UBSan, or plain at -O2."""
    exe = os.path.join(tempfile.mkdtemp(prefix="geom_check_"), "geom_check")
    flags = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
             if sanitize else ["-O2"])
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags +
                       ["-I", CSRC, os.path.join(ROOT, "tests", "abi", "geom_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def header_constants():
    """{'tile': kMatchTile, 'block': kBlockHyp} as the header has them."""
    out = subprocess.run([check_program(False), "info"], capture_output=True, text=True, check=True).stdout.split()
    return {out[0]: int(out[1]), out[2]: int(out[3])}


def write_scene(d, loc, off, pairs, matches, model, threshold, iterations, seed):
    params = np.zeros(4, np.int32)
    params[0], params[1] = MODELS[model], iterations
    params[2:3].view(np.uint32)[0] = seed
    params[3:4].view(np.float32)[0] = threshold
    params.tofile(os.path.join(d, "params.bin"))
    np.ascontiguousarray(loc, np.float32).tofile(os.path.join(d, "loc.bin"))
    np.ascontiguousarray(off, np.int64).tofile(os.path.join(d, "offsets.bin"))
    np.ascontiguousarray(pairs, np.int32).reshape(-1, 2).tofile(os.path.join(d, "pairs.bin"))
    ms = [np.ascontiguousarray(m, np.int32).reshape(-1, 2) for m in matches]
    (np.concatenate(ms) if ms else np.zeros((0, 2), np.int32)).astype(np.int32).tofile(os.path.join(d, "matches.bin"))
    np.array([len(m) for m in ms], np.int32).tofile(os.path.join(d, "counts.bin"))
    return [len(m) for m in ms]


def host_estimate(loc, off, pairs, matches, model, threshold, iterations, seed, sanitize=False):
    """sgeo::estimate_host on one pair list: (models [npairs][3][3] float32, inliers [npairs] int32,
    masks: one bool array per pair), the layout SiftContext.estimate_batch returns."""
    with tempfile.TemporaryDirectory(prefix="geom_scene_") as d:
        counts = write_scene(d, loc, off, pairs, matches, model, threshold, iterations, seed)
        r = subprocess.run([check_program(sanitize), "run", d], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        models = np.fromfile(os.path.join(d, "models.bin"), np.float32).reshape(len(counts), 3, 3)
        inliers = np.fromfile(os.path.join(d, "inliers.bin"), np.int32)
        mask = np.fromfile(os.path.join(d, "mask.bin"), np.uint8)
    offs = np.concatenate([[0], np.cumsum(counts)])
    assert len(mask) == offs[-1] and set(np.unique(mask)) <= {0, 1}
    return models, inliers, [mask[offs[p]:offs[p + 1]].astype(bool) for p in range(len(counts))]


def _as_sets(x1, x2, planted, rng):
    """Two sets and their matches from corresponding points: the matches come in random order of
    the correspondences, set b's rows are permuted, {i, j} ascending in i."""
    n = len(x1)
    order = rng.permutation(n)
    x1, x2, planted = x1[order], x2[order], planted[order]
    perm = rng.permutation(n)            # set b row perm[k] holds x2[k]
    lb = np.zeros_like(x2)
    lb[perm] = x2
    matches = np.stack([np.arange(n), perm], 1).astype(np.int32)
    return x1.astype(np.float32), lb.astype(np.float32), matches, planted


@functools.lru_cache(maxsize=None)
def h_scene(seed=101, n=300, n_planted=180):
    """n matches in 640 x 480, n_planted of them under a mild projective map with +-0.3 px uniform
    noise, the rest uniform random.  (set a [n][2], set b [n][2], matches [n][2], planted [n])"""
    rng = np.random.Generator(np.random.PCG64(seed))
    P = np.array([[1.02, 0.03, 8.0], [-0.02, 0.98, -5.0], [2e-5, -1e-5, 1.0]])
    x1 = rng.uniform([0, 0], [640, 480], (n, 2))
    h = np.c_[x1, np.ones(n)] @ P.T
    x2 = h[:, :2] / h[:, 2:] + rng.uniform(-0.3, 0.3, (n, 2))
    planted = np.arange(n) < n_planted
    x2[~planted] = rng.uniform([0, 0], [640, 480], (n - n_planted, 2))
    return _as_sets(x1, x2, planted, rng)


@functools.lru_cache(maxsize=None)
def f_scene(seed=202, n=400, n_planted=280):
    """n matches, n_planted of them from two pinhole views (f = 500, centre (320, 240)) of points at
    depth 4-8 with +-0.3 px uniform noise, the rest uniform random."""
    rng = np.random.Generator(np.random.PCG64(seed))
    K = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
    x1 = rng.uniform([0, 0], [640, 480], (n, 2))
    X = (np.c_[x1, np.ones(n)] @ np.linalg.inv(K).T) * rng.uniform(4, 8, (n, 1))
    ay, ax = 0.08, -0.03
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    c = (X @ (Ry @ Rx).T + np.array([0.6, 0.05, 0.1])) @ K.T
    x2 = c[:, :2] / c[:, 2:] + rng.uniform(-0.3, 0.3, (n, 2))
    x1 = x1 + rng.uniform(-0.3, 0.3, (n, 2))
    planted = np.arange(n) < n_planted
    x2[~planted] = rng.uniform([0, 0], [640, 480], (n - n_planted, 2))
    return _as_sets(x1, x2, planted, rng)


FRONT = 5   # buffer rows in front of the first set
REAL = 0    # the planted scene's position in pair_list()


@functools.lru_cache(maxsize=None)
def pair_list(model):
    """The planted scene of `model` and the edge pairs around it, one call's worth:
    (loc, offsets, pairs, matches, planted mask of pair REAL).  Sets: 0, 1 = the scene (set 0
    starts at buffer row FRONT), 2 = ten rows at one point, 3 = empty."""
    la, lb, m, planted = h_scene() if model == "H" else f_scene()
    S = MIN_SAMPLE[model]
    same = np.tile(np.array([[100.5, 50.25]], np.float32), (10, 1))
    front = np.full((FRONT, 2), 7777.0, np.float32)
    loc = np.concatenate([front, la, lb, same])
    off = np.array([FRONT, FRONT + len(la), FRONT + len(la) + len(lb), len(loc), len(loc)], np.int64)
    good = m[planted]
    rev = m[:, ::-1][np.argsort(m[:, 1], kind="stable")]
    ident = np.stack([np.arange(S + 2)] * 2, 1).astype(np.int32)
    none = np.zeros((0, 2), np.int32)
    pairs = [(0, 1), (0, 1), (1, 0), (0, 1),            # the scene; an empty pair between real ones;
             (0, 1), (0, 1), (0, 1), (0, 1),            # (b, a); the repeat; m = 0, S - 1, S, S + 1
             (2, 2), (3, 0)]                            # all one point; an empty set
    matches = [m, none, rev, m, none, good[:S - 1], good[:S], good[:S + 1], ident, none]
    return loc, off, pairs, matches, planted


def predicate64(model, M, x1, x2):
    """The inlier test restated in float64 (NumPy): the error of every match -- H: the larger
    coordinate difference of H x1 and x2; F: the Sampson error."""
    M = M.astype(np.float64).reshape(3, 3)
    a = np.c_[x1.astype(np.float64), np.ones(len(x1))]
    b = np.c_[x2.astype(np.float64), np.ones(len(x2))]
    with np.errstate(all="ignore"):
        if model == "H":
            h = a @ M.T
            return np.abs(h[:, :2] / h[:, 2:] - b[:, :2]).max(1)
        f = a @ M.T          # F x1
        t = b @ M            # F' x2
        return (b * f).sum(1) ** 2 / (f[:, 0] ** 2 + f[:, 1] ** 2 + t[:, 0] ** 2 + t[:, 1] ** 2)
