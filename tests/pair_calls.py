"""Inputs and call lists shared by tests/test_gpu_pair_calls_interleaved.py and
tests/pair_host_trace.py: every call family that runs over the grouped pair matcher's shared host
path (csrc/sgpu_pairs.cpp), on one small list of sets and on one small extracted batch.

Sets of 0, 1, 130, 300 and 64 rows: an empty set, a single row, one row past a 128-row panel, more
than two 128-column tiles, and fewer rows than top = 64 allows to drop.  The 300-row set is the
scene; the others start with noisy copies of its first rows, seen through one homography."""
import functools

import numpy as np

from sift_synth import quantize, synth_descriptors, synth_image

SIZES = [0, 1, 130, 300, 64]
EMPTY, ONE, PANEL, SCENE, FEW = range(5)
COPIES = {ONE: 1, PANEL: 60, FEW: 40}
PAIRS = [(SCENE, PANEL), (PANEL, SCENE), (SCENE, FEW), (FEW, PANEL), (ONE, SCENE), (EMPTY, SCENE),
         (SCENE, EMPTY), (SCENE, SCENE), (PANEL, FEW)]
TOP = 64
SEED = 3
VIEW = np.array([[0.98, -0.05, 14.0], [0.04, 1.01, -9.0], [2e-5, -1e-5, 1.0]])


def _through(M, x):
    c = np.c_[x, np.ones(len(x))] @ M.T
    return c[:, :2] / c[:, 2:]


@functools.lru_cache(maxsize=None)
def sets():
    """(u8 descriptors [rows][128], locations [rows][2], scales [rows], offsets, per-pair H)."""
    rng = np.random.Generator(np.random.PCG64(7300))
    scene = synth_descriptors(SIZES[SCENE], 7301)
    at = rng.uniform([0, 0], [640, 480], (SIZES[SCENE], 2))
    desc, loc = [], []
    for s, n in enumerate(SIZES):
        k = COPIES.get(s, 0)
        d = scene if s == SCENE else synth_descriptors(n, 7302 + s, base=scene, n_dup=k)
        l = at.copy() if s == SCENE else rng.uniform([0, 0], [640, 480], (n, 2))
        if k:
            l[:k] = _through(VIEW, at[:k]) + rng.uniform(-0.3, 0.3, (k, 2))
        desc.append(quantize(d))
        loc.append(l)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    buf = np.ascontiguousarray(np.concatenate(desc), np.uint8)
    loc = np.ascontiguousarray(np.concatenate(loc), np.float32)
    scale = rng.uniform(1.0, 20.0, len(buf)).astype(np.float32)
    view = {s: (np.eye(3) if s == SCENE else VIEW) for s in range(len(SIZES))}
    H = np.stack([view[b] @ np.linalg.inv(view[a]) for a, b in PAIRS]).astype(np.float32)
    return buf, loc, scale, off, H


def set_calls(putative, overflow_cap):
    """The interleaving test's six calls, in its order: (name, f(ctx)).  putative: what match_batch
    returns for PAIRS (the estimator's input); overflow_cap: a cap below their total."""
    buf, loc, scale, off, H = sets()
    return [
        ("match_batch", lambda c: c.match_batch(buf, off, PAIRS)),
        ("verify_batch", lambda c: c.verify_batch(buf, loc, off, PAIRS, True, True, seed=SEED)),
        ("prematch_batch", lambda c: c.prematch_batch(buf, scale, off, PAIRS, top=TOP, matches=True)),
        ("match_batch_guided", lambda c: c.match_batch_guided(buf, loc, off, PAIRS, H=H)),
        ("estimate_batch_refined",
         lambda c: c.estimate_batch_refined(loc, off, PAIRS, putative, "H", seed=SEED)),
        ("match_batch overflow", lambda c: c.match_batch(buf, off, PAIRS, cap=overflow_cap)),
    ]


# ---- the image side: 4 views of one 160 x 120 image, each rolled by (rows, columns)
ROLLS = [(0, 0), (5, 9), (3, -4), (11, 2)]
IMAGE_PAIRS = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 0)]


def views():
    img = synth_image(160, 120, 61)
    return np.stack([np.roll(img, s, axis=(0, 1)) for s in ROLLS])


def image_H():
    """The translation between the views of every image pair."""
    H = np.tile(np.eye(3, dtype=np.float32), (len(IMAGE_PAIRS), 1, 1))
    for p, (a, b) in enumerate(IMAGE_PAIRS):
        H[p, 0, 2] = ROLLS[b][1] - ROLLS[a][1]
        H[p, 1, 2] = ROLLS[b][0] - ROLLS[a][0]
    return H


def image_calls():
    H = image_H()
    return [
        ("match_images", lambda c: c.match_images(IMAGE_PAIRS)),
        ("verify_images", lambda c: c.verify_images(IMAGE_PAIRS, True, True, seed=SEED)),
        ("prematch_images", lambda c: c.prematch_images(IMAGE_PAIRS, top=TOP, matches=True)),
        ("match_images_guided", lambda c: c.match_images_guided(IMAGE_PAIRS, H=H)),
    ]
