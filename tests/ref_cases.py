"""Inputs shared by tests/test_ref_kernels.py and tests/make_ref_golden.py: every case is built
from seeds, so a fixture holds results only."""
from __future__ import annotations

import functools

import numpy as np

import oracle_py as O
import structured_images as SI
from sgpu_types import default_options
from sift_synth import (quantize, synth_descriptors, synth_guided_scene, synth_image,
                        synth_tie_scene)

# ---- matcher -------------------------------------------------------------------------------
TIE_COLS_SMALL = [(5, 34), (40, 66), (3, 99), (31, 32), (7, 39)]
TIE_COLS_LARGE = [(200, 129), (130, 2), (4000, 33), (8999, 1), (640, 4064), (7000, 5000)]
THRESHOLDS = [(0.7, 0.8), (0.5, 0.6), (1.0, 1.0), (0.9, 0.95), (0.7, 1.5)]


def _sized(n1, n2, dup):
    d1 = synth_descriptors(n1, 10 * n1 + n2)
    d2 = synth_descriptors(n2, 10 * n2 + n1 + 1, base=d1, n_dup=min(dup, n1, n2))
    return quantize(d1), quantize(d2)


@functools.lru_cache(maxsize=None)
def match_case(name):
    """(q1, q2, dict(distmax, ratiomax)) of a plain matcher case; each runs with mbm 0 and 1."""
    if name.startswith("size_"):
        n1, n2, dup = map(int, name.split("_")[1:])
        return _sized(n1, n2, dup) + ({},)
    if name == "tie_70x100":
        q1, q2, _ = synth_tie_scene(70, 100, 21, TIE_COLS_SMALL, [(60, 61)])
        return q1, q2, dict(distmax=2.0, ratiomax=1.5)
    if name == "tie_3000x9000":
        q1, q2, _ = synth_tie_scene(3000, 9000, 12000, TIE_COLS_LARGE, [(60, 61), (1, 2995)])
        return q1, q2, dict(distmax=2.0, ratiomax=1.5)
    if name == "duplicated_rows":
        base = quantize(synth_descriptors(400, 5))
        return base, np.concatenate([base, base[:200]]), {}
    if name == "all_zero":
        z = np.zeros((50, 128), np.uint8)
        return z, z.copy(), {}
    if name.startswith("thresholds_"):
        distmax, ratiomax = THRESHOLDS[int(name.split("_")[1])]
        d1 = synth_descriptors(1500, 71)
        d2 = synth_descriptors(1800, 72, base=d1, n_dup=700)
        return quantize(d1), quantize(d2), dict(distmax=distmax, ratiomax=ratiomax)
    raise KeyError(name)


MATCH_SMALL = ["size_1_1_0", "size_1_700_0", "size_700_1_0", "tie_70x100", "all_zero"]
MATCH_LIVE = MATCH_SMALL + ["size_257_1000_100", "tie_3000x9000", "duplicated_rows"] + [
    f"thresholds_{i}" for i in range(len(THRESHOLDS))]

GUIDED_SCENES = [(300, 250, 32.0, 16.0, 1), (301, 257, 8.0, 1.0, 1), (173, 190, 32.0, 16.0, 0),
                 (9, 7, 64.0, 1e3, 1)]


@functools.lru_cache(maxsize=None)
def guided_case(name):
    """(q1, q2, loc1, loc2, H, F, dict(hdistmax, fdistmax, mbm, distmax, ratiomax))."""
    if name == "block_rule":
        # tests/test_oracle.py test_guided_block_rule_matters: only the 8-row block rule gives
        # row r a positive value at column j
        q1, q2, l1, l2, H, F = synth_guided_scene(64, 40, 9, n_dup=0)
        self_dot = (q1.astype(np.int64) ** 2).sum(1)
        r = int(next(i for i in range(1, 64) if self_dot[i] > 262144 and i % 8))
        mate, j = r - r % 8, 17
        q2[j] = q1[r]
        x = H.astype(np.float64) @ np.array([l1[mate, 0], l1[mate, 1], 1.0])
        l2[j] = (x[:2] / x[2]).astype(np.float32)
        return q1, q2, l1, l2, H, F, dict(hdistmax=32.0, fdistmax=16.0, mbm=0, distmax=2.0,
                                          ratiomax=1.0, planted=(r, j))
    n1, n2, hd, fd, mbm = GUIDED_SCENES[int(name.split("_")[1])]
    return synth_guided_scene(n1, n2, n1 + n2) + (dict(hdistmax=hd, fdistmax=fd, mbm=mbm,
                                                         distmax=0.7, ratiomax=0.8),)


GUIDED_SMALL = ["scene_3", "block_rule"]
GUIDED_LIVE = [f"scene_{i}" for i in range(len(GUIDED_SCENES))] + ["block_rule"]

# ---- images ----------------------------------------------------------------------------------
TIE_SIZE = (203, 97)
FLOAT_IMAGES = {"synth_160x120": (160, 120, 1), "synth_203x97": (203, 97, 2)}
FILTER_SHAPES = [(16, 16), (131, 37), (300, 140)]


# The orientation tie rules T2 and T4 (oracle/sift_oracle.cpp) are reached by no tie image at
# 203 x 97, and at 320 x 240 by these levels only (8 keypoints of checker8, one of blobs_int).
TIE_ORIENTATION_EXTRA = {"checker8@320x240": [(0, 1)], "blobs_int@320x240": [(0, 0)]}
ALL_LEVELS = [(o, j) for o in range(2) for j in range(3)]


@functools.lru_cache(maxsize=None)
def image(name):
    if name in FLOAT_IMAGES:
        return synth_image(*FLOAT_IMAGES[name])
    if "@" in name:
        base, size = name.split("@")
        return SI.image(base, *map(int, size.split("x")))
    return SI.image(name, *TIE_SIZE)


@functools.lru_cache(maxsize=None)
def levels(name, max_orientation=2):
    """The oracle's stages of every level of the first two octaves of image `name` (of the
    levels listed in TIE_ORIENTATION_EXTRA for those images)."""
    opts = default_options(max_orientation=max_orientation)
    return {(o, j): O.level_stages(image(name), o, j, opts)
            for o, j in TIE_ORIENTATION_EXTRA.get(name, ALL_LEVELS)}


def unit_image(w, h, seed):
    """A float image in [0, 1] of any size (filters take the pyramid's float levels)."""
    return synth_image(w, h, seed).astype(np.float32) / np.float32(255.0)


def filter_sigmas():
    """Every (sigma, -d) of the schedule at -d 3 and -d 5, duplicates dropped."""
    out = []
    for d in (3, 5):
        for s in O.filter_sigmas(d):
            if s not in out:
                out.append(s)
    return out


def key_image(w, h, count, seed):
    """A synthetic key image [h, w, 4] with `count` keys (+-1) at random interior pixels, a few
    of them in the first and last interior columns and rows."""
    rng = np.random.Generator(np.random.PCG64(seed))
    k = np.zeros((h, w, 4), np.float32)
    cells = rng.permutation((h - 2) * (w - 2))[:count]
    rows, cols = cells // (w - 2) + 1, cells % (w - 2) + 1
    k[rows, cols, 0] = rng.choice([-1.0, 1.0], size=len(cells))
    k[rows, cols, 1:] = rng.uniform(-0.5, 0.5, (len(cells), 3))
    return k


# (width, height, keys): histogram widths w / 4 = 127, 128, 129 (both sides of the 128-wide
# InitHist block) and list lengths 127, 128, 129 and 300 (the 128-wide ListGen block); 200 x 97
# is the first octave of the 203 x 97 images
LIST_CASES = [(200, 97, 5), (508, 9, 127), (512, 9, 128), (516, 9, 129), (516, 12, 300),
              (16, 16, 3)]
