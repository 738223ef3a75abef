"""Driver of tests/abi/geom_refine_check.cpp, the stand-alone program that runs sgeo::refine_host
(csrc/sift_geom.h): the host reference of the estimator's local refinement, shared by
test_geom_refine.py (CPU) and test_gpu_estimate_refine.py (device).  The scenes are geom_scenes'."""
import functools
import os
import re
import subprocess
import tempfile

import numpy as np

import geom_scenes as G

# the thresholds at which the unrefined model misses planted matches
H_TIGHT = dict(model="H", threshold=0.45, iterations=512, seed=11)
F_TIGHT = dict(model="F", threshold=0.15, iterations=1024, seed=12)
STOPS = ("budget", "fixed point", "rejected", "invalid", "no model")


@functools.lru_cache(maxsize=None)
def check_program(sanitize: bool) -> str:
    """geom_refine_check built with g++, no contraction; under ASan + UBSan, or plain at -O2."""
    exe = os.path.join(tempfile.mkdtemp(prefix="geom_refine_check_"), "geom_refine_check")
    flags = (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
             if sanitize else ["-O2"])
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags +
                       ["-I", G.CSRC, os.path.join(G.ROOT, "tests", "abi", "geom_refine_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def header_constants():
    """{'sweeps': kJacobiSweeps, 'lanes': kRefineLanes} as the header has them."""
    out = subprocess.run([check_program(False), "info"], capture_output=True, text=True, check=True).stdout.split()
    return {out[0]: int(out[1]), out[2]: int(out[3])}


def host_refine(loc, off, pairs, matches, model, threshold, iterations, seed, rounds, sanitize=False,
                info=None):
    """sgeo::refine_host on one pair list: (models [npairs][3][3] float32, inliers [npairs] int32,
    masks: one bool array per pair, accepted rounds [npairs] int32), the layout
    SiftContext.estimate_batch_refined returns.  info (a dict) receives 'stops', the stop reason of
    every pair, and 'sweeps', the Jacobi sweeps the scene's refit matrices needed."""
    with tempfile.TemporaryDirectory(prefix="geom_scene_") as d:
        counts = G.write_scene(d, loc, off, pairs, matches, model, threshold, iterations, seed)
        r = subprocess.run([check_program(sanitize), "run", d, str(rounds)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        models = np.fromfile(os.path.join(d, "models.bin"), np.float32).reshape(len(counts), 3, 3)
        inliers = np.fromfile(os.path.join(d, "inliers.bin"), np.int32)
        mask = np.fromfile(os.path.join(d, "mask.bin"), np.uint8)
        done = np.fromfile(os.path.join(d, "rounds.bin"), np.int32)
    offs = np.concatenate([[0], np.cumsum(counts)])
    assert len(mask) == offs[-1] and set(np.unique(mask)) <= {0, 1} and len(done) == len(counts)
    if info is not None:
        stops = re.findall(r"^pair (\d+) rounds (\d+) stop (.+)$", r.stdout, re.M)
        assert [int(s[0]) for s in stops] == list(range(len(counts)))
        assert [int(s[1]) for s in stops] == done.tolist() and all(s[2] in STOPS for s in stops)
        info["stops"] = [s[2] for s in stops]
        info["sweeps"] = int(re.search(r"^sweeps_scene (\d+)$", r.stdout, re.M).group(1))
    masks = [mask[offs[p]:offs[p + 1]].astype(bool) for p in range(len(counts))]
    return models, inliers, masks, done
