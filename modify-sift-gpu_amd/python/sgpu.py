"""ctypes binding of the C ABI (include/sgpu.h) of lib/libsiftgpu.so.

The binding fails loudly when the library or a usable GPU is missing: there is no CPU path.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes
import os
import subprocess

import numpy as np

from sgpu_types import SgpuOptions, SgpuVerifyParams, default_options

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# SGPU_LIB_PATH: an experiment build of the same library (tests/build_variant.sh); default: the
# in-tree product build
LIB_PATH = os.environ.get("SGPU_LIB_PATH") or os.path.join(PKG, "lib", "libsiftgpu.so")

SGPU_OK, SGPU_EINVAL, SGPU_ENODEV, SGPU_ENOMEM, SGPU_ERANGE = 0, -1, -2, -3, -4
SGPU_INPUT_HOST, SGPU_INPUT_DEVICE, SGPU_INPUT_STAGED = 0, 1, 2
SGPU_TRACK_NONE, SGPU_TRACK_INCONSISTENT = -1, -2

# every extern "C" symbol include/sgpu.h declares (tests check the library exports them all)
C_API = [
    "sgpu_default_options", "sgpu_parse_args", "sgpu_ctx_create", "sgpu_ctx_destroy",
    "sgpu_ctx_set_options", "sgpu_last_error", "sgpu_device_count", "sgpu_extract",
    "sgpu_extract_f32", "sgpu_stage_input", "sgpu_feature_count", "sgpu_feature_total", "sgpu_copy_features",
    "sgpu_device_features", "sgpu_match", "sgpu_quantize_descriptors", "sgpu_last_timing",
    "sgpu_debug_geometry", "sgpu_debug_gaussian", "sgpu_debug_candidates",
    "sgpu_debug_set_flags", "sgpu_comm_unique_id", "sgpu_comm_init", "sgpu_comm_allgather_i32",
    "sgpu_comm_allreduce_f64", "sgpu_extract_keypoints", "sgpu_match_guided", "sgpu_extract_color",
    "sgpu_match_shard_begin", "sgpu_match_shard_end", "sgpu_match_sharded",
    "sgpu_extract_stream", "sgpu_host_alloc", "sgpu_host_free", "sgpu_reserve",
    "sgpu_debug_alloc_count", "sgpu_last_pyramid_launches", "sgpu_set_stage_timing",
    "sgpu_set_host_output", "sgpu_debug_set_schedule", "sgpu_debug_set_match_prune",
    "sgpu_quantize_descriptors_gpu", "sgpu_feature_descriptors_u8", "sgpu_copy_features_u8",
    "sgpu_match_batch", "sgpu_match_images", "sgpu_debug_match_plan_stats",
    "sgpu_debug_set_duo_strips", "sgpu_debug_pyramid_plan", "sgpu_debug_set_feature_queue",
    "sgpu_match_batch_guided", "sgpu_match_images_guided",
    "sgpu_estimate_batch", "sgpu_estimate_images",
    "sgpu_estimate_batch_refined", "sgpu_estimate_images_refined",
    "sgpu_default_verify_params", "sgpu_verify_batch", "sgpu_verify_images",
    "sgpu_select_top_scale_batch", "sgpu_select_top_scale_images",
    "sgpu_prematch_batch", "sgpu_prematch_images",
    "sgpu_debug_set_top_level", "sgpu_debug_top_level_at",
    "sgpu_tracks_batch", "sgpu_tracks_images",
    "sgpu_pose_batch", "sgpu_pose_images",
]

# launch kinds of SiftContext.pyramid_plan() (SGPU_PLAN_* of sgpu.h, in their order)
PLAN_KINDS = ("level", "tile", "two", "tile_two", "tile_duo", "tile_duo_one", "duo", "trio")

_LIB = None


def build():
    subprocess.check_call(["make", "-C", PKG, "-j8"])


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: build it with `make -C {PKG}`")
        L = ctypes.CDLL(LIB_PATH)
        P, c = ctypes.POINTER, ctypes
        vp = c.c_void_p
        L.sgpu_default_options.argtypes = [P(SgpuOptions)]
        L.sgpu_parse_args.argtypes = [P(SgpuOptions), c.c_int, P(c.c_char_p), P(c.c_int)]
        L.sgpu_ctx_create.argtypes = [c.c_int, P(SgpuOptions), P(vp)]
        L.sgpu_ctx_destroy.argtypes = [vp]
        L.sgpu_ctx_set_options.argtypes = [vp, P(SgpuOptions)]
        L.sgpu_last_error.argtypes = [vp]
        L.sgpu_last_error.restype = c.c_char_p
        L.sgpu_extract.argtypes = [vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int]
        L.sgpu_stage_input.argtypes = [vp, vp, c.c_int, c.c_int, c.c_int, c.c_int]
        L.sgpu_reserve.argtypes = [vp, c.c_int, c.c_int, c.c_int, c.c_int]
        L.sgpu_debug_alloc_count.argtypes = []
        L.sgpu_debug_alloc_count.restype = c.c_longlong
        L.sgpu_last_pyramid_launches.argtypes = [vp, P(c.c_int)]
        L.sgpu_set_stage_timing.argtypes = [vp, c.c_int]
        L.sgpu_set_host_output.argtypes = [vp, vp, vp, c.c_int]
        L.sgpu_extract_f32.argtypes = [vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int]
        L.sgpu_feature_count.argtypes = [vp, c.c_int]
        L.sgpu_feature_total.argtypes = [vp]
        L.sgpu_feature_total.restype = c.c_int64
        L.sgpu_copy_features.argtypes = [vp, c.c_int, vp, vp]
        L.sgpu_device_features.argtypes = [vp, P(vp), P(vp), P(vp)]
        L.sgpu_match.argtypes = [vp, vp, c.c_int, vp, c.c_int, c.c_float, c.c_float, c.c_int,
                                 c.c_int, vp, c.c_int]
        L.sgpu_match_guided.argtypes = [vp, vp, c.c_int, vp, c.c_int, vp, vp, vp, vp, c.c_float,
                                        c.c_float, c.c_float, c.c_float, c.c_int, c.c_int, vp,
                                        c.c_int]
        L.sgpu_extract_color.argtypes = [vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int]
        L.sgpu_quantize_descriptors.argtypes = [vp, c.c_size_t, vp]
        L.sgpu_last_timing.argtypes = [vp, vp, c.c_int]
        L.sgpu_debug_set_flags.argtypes = [vp, c.c_int]
        L.sgpu_debug_set_schedule.argtypes = [vp, c.c_int, c.c_int]
        L.sgpu_debug_set_match_prune.argtypes = [vp, c.c_int]
        L.sgpu_debug_set_duo_strips.argtypes = [vp, c.c_int]
        L.sgpu_debug_set_feature_queue.argtypes = [vp, c.c_int]
        L.sgpu_debug_set_top_level.argtypes = [vp, c.c_int]
        L.sgpu_debug_top_level_at.argtypes = [vp, c.c_int, c.c_int, c.c_int, c.c_int, vp]
        L.sgpu_debug_geometry.argtypes = [vp, P(c.c_int), vp, c.c_int]
        L.sgpu_debug_gaussian.argtypes = [vp, c.c_int, c.c_int, c.c_int, vp]
        L.sgpu_debug_candidates.argtypes = [vp, vp, vp, c.c_int, P(c.c_int)]
        L.sgpu_extract_keypoints.argtypes = [vp, c.c_int, vp, c.c_int, c.c_int]
        L.sgpu_comm_unique_id.argtypes = [vp, c.c_int]
        L.sgpu_comm_init.argtypes = [vp, c.c_int, c.c_int, vp, c.c_int]
        L.sgpu_comm_allgather_i32.argtypes = [vp, vp, c.c_int, vp]
        L.sgpu_comm_allreduce_f64.argtypes = [vp, vp, c.c_int, c.c_int]
        L.sgpu_match_shard_begin.argtypes = [vp, vp, c.c_int, c.c_int, vp, c.c_int, c.c_float,
                                             c.c_float, c.c_int, vp, vp, c.c_int]
        L.sgpu_match_shard_end.argtypes = [vp, c.c_int, c.c_int, vp, c.c_int, c.c_int, c.c_float,
                                           c.c_float, c.c_int, c.c_int, vp]
        L.sgpu_match_sharded.argtypes = [vp, vp, c.c_int, c.c_int, vp, c.c_int, c.c_float,
                                         c.c_float, c.c_int, c.c_int, vp, c.c_int]
        L.sgpu_extract_stream.argtypes = [vp, P(vp), c.c_int, c.c_int, c.c_int, c.c_int, c.c_int,
                                          vp, vp, c.c_int64, vp]
        L.sgpu_host_alloc.argtypes = [c.c_size_t]
        L.sgpu_host_alloc.restype = vp
        L.sgpu_host_free.argtypes = [vp]
        L.sgpu_quantize_descriptors_gpu.argtypes = [vp, vp, c.c_size_t, vp, c.c_int]
        L.sgpu_feature_descriptors_u8.argtypes = [vp, P(vp)]
        L.sgpu_copy_features_u8.argtypes = [vp, c.c_int, vp]
        L.sgpu_match_batch.argtypes = [vp, vp, vp, c.c_int, vp, c.c_int, c.c_float, c.c_float,
                                       c.c_int, c.c_int, vp, c.c_int64, vp, c.c_int]
        L.sgpu_match_images.argtypes = [vp, vp, c.c_int, c.c_float, c.c_float, c.c_int, c.c_int,
                                        vp, c.c_int64, vp]
        L.sgpu_match_batch_guided.argtypes = [vp, vp, vp, vp, c.c_int, vp, c.c_int, vp, vp,
                                              c.c_float, c.c_float, c.c_float, c.c_float,
                                              c.c_int, c.c_int, vp, c.c_int64, vp, c.c_int]
        L.sgpu_match_images_guided.argtypes = [vp, vp, c.c_int, vp, vp, c.c_float, c.c_float,
                                               c.c_float, c.c_float, c.c_int, c.c_int, vp,
                                               c.c_int64, vp]
        L.sgpu_estimate_batch.argtypes = [vp, vp, vp, c.c_int, vp, c.c_int, vp, vp, c.c_int,
                                          c.c_float, c.c_int, c.c_uint32, vp, vp, vp, c.c_int]
        L.sgpu_estimate_images.argtypes = [vp, vp, c.c_int, vp, vp, c.c_int, c.c_float, c.c_int,
                                           c.c_uint32, vp, vp, vp]
        L.sgpu_estimate_batch_refined.argtypes = [vp, vp, vp, c.c_int, vp, c.c_int, vp, vp,
                                                  c.c_int, c.c_float, c.c_int, c.c_uint32,
                                                  c.c_int, vp, vp, vp, vp, c.c_int]
        L.sgpu_estimate_images_refined.argtypes = [vp, vp, c.c_int, vp, vp, c.c_int, c.c_float,
                                                   c.c_int, c.c_uint32, c.c_int, vp, vp, vp, vp]
        L.sgpu_default_verify_params.argtypes = [P(SgpuVerifyParams)]
        L.sgpu_default_verify_params.restype = None
        L.sgpu_verify_batch.argtypes = [vp, vp, vp, vp, c.c_int, vp, c.c_int, P(SgpuVerifyParams),
                                        vp, vp, vp, vp, vp, vp, c.c_int64, vp, c.c_int]
        L.sgpu_verify_images.argtypes = [vp, vp, c.c_int, P(SgpuVerifyParams), vp, vp, vp, vp, vp,
                                         vp, c.c_int64, vp]
        L.sgpu_select_top_scale_batch.argtypes = [vp, vp, c.c_int, vp, c.c_int, c.c_int, vp, vp,
                                                  c.c_int]
        L.sgpu_select_top_scale_images.argtypes = [vp, c.c_int, vp, vp]
        L.sgpu_prematch_batch.argtypes = [vp, vp, vp, c.c_int, vp, c.c_int, vp, c.c_int, c.c_int,
                                          c.c_float, c.c_float, c.c_int, vp, vp, c.c_int64, c.c_int]
        L.sgpu_prematch_images.argtypes = [vp, vp, c.c_int, c.c_int, c.c_float, c.c_float, c.c_int,
                                           vp, vp, c.c_int64]
        L.sgpu_tracks_batch.argtypes = [vp, vp, c.c_int, vp, c.c_int, vp, vp, c.c_int, vp, vp, vp, vp]
        L.sgpu_tracks_images.argtypes = [vp, vp, c.c_int, vp, vp, c.c_int, vp, vp, vp, vp]
        L.sgpu_pose_batch.argtypes = [vp, vp, vp, c.c_int, vp, vp, c.c_int, vp, vp, vp, c.c_float,
                                      c.c_float, vp, vp, vp, vp, vp, c.c_int]
        L.sgpu_pose_images.argtypes = [vp, vp, vp, c.c_int, vp, vp, vp, c.c_float, c.c_float, vp, vp,
                                       vp, vp, vp]
        L.sgpu_debug_match_plan_stats.argtypes = [vp, vp]
        L.sgpu_debug_pyramid_plan.argtypes = [vp, vp, c.c_int]
        _LIB = L
    return _LIB


class PinnedArray:
    """A numpy view of page-locked host memory (sgpu_host_alloc): the form of host buffer whose
    copies overlap the kernels in sgpu_extract_stream.  Freed with .free() or on collection."""

    def __init__(self, shape, dtype):
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        self._p = lib().sgpu_host_alloc(max(n, 1))
        if not self._p:
            raise MemoryError(f"sgpu_host_alloc({n}) failed")
        buf = (ctypes.c_uint8 * max(n, 1)).from_address(self._p)
        self.array = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if self._p:
            self.array = None
            lib().sgpu_host_free(self._p)
            self._p = None

    def __del__(self):
        self.free()


def match_shard_end(col_best_all: np.ndarray, row_match: np.ndarray, row_begin: int,
                    distmax=0.7, ratiomax=0.8, mbm=1, max_match=None) -> np.ndarray:
    """Host-side merge of the shards' column states ([nshards][n2][3] int32, rank order) plus
    this shard's row decisions -> this shard's pairs {global i, j} (sgpu_match_shard_end; no
    device involved)."""
    cb = np.ascontiguousarray(col_best_all, np.int32)
    if cb.ndim == 2:
        cb = cb[None]
    rm = np.ascontiguousarray(row_match, np.int32)
    ns, n2 = len(rm), cb.shape[1]
    max_match = ns if max_match is None else max_match
    out = np.zeros((max(max_match, 1), 2), np.int32)
    m = lib().sgpu_match_shard_end(cb.ctypes.data, cb.shape[0], n2, rm.ctypes.data, ns,
                                   row_begin, distmax, ratiomax, mbm, max_match, out.ctypes.data)
    if m < 0:
        raise RuntimeError(f"sgpu_match_shard_end failed ({m})")
    return out[:m].copy()


def comm_unique_id() -> bytes:
    """A fresh RCCL communicator id (rank 0 creates it, the launcher distributes it)."""
    buf = (ctypes.c_uint8 * 128)()
    rc = lib().sgpu_comm_unique_id(buf, 128)
    if rc != SGPU_OK:
        raise RuntimeError(f"sgpu_comm_unique_id failed ({rc})")
    return bytes(buf)


def device_count() -> int:
    return lib().sgpu_device_count()


def quantize(desc: np.ndarray) -> np.ndarray:
    d = np.ascontiguousarray(desc, np.float32)
    out = np.empty(d.shape, np.uint8)
    lib().sgpu_quantize_descriptors(d.ctypes.data, d.size, out.ctypes.data)
    return out


def quantize_gpu(desc: np.ndarray, ctx: "SiftContext | None" = None) -> np.ndarray:
    """quantize() on the device (sgpu_quantize_descriptors_gpu, host pointers): the same bytes.
    Without a context a temporary one on device 0 is used."""
    own = ctx is None
    if own:
        ctx = SiftContext(0)
    try:
        return ctx.quantize_gpu(desc)
    finally:
        if own:
            ctx.close()


# What tracks_batch / tracks_images return: track_of_row [rows] int32 (the track id, SGPU_TRACK_NONE
# or SGPU_TRACK_INCONSISTENT), offsets [T + 1] int64 and rows [offsets[T]] int32 (track t's rows =
# rows[offsets[t]:offsets[t + 1]], ascending), stats [4] int64 = (components of >= 2 rows, tracks,
# inconsistent components, short components of >= 2 rows).
Tracks = collections.namedtuple("Tracks", "track_of_row offsets rows stats")
# what pose_batch / pose_images return: R [npairs][3][3], t [npairs][3] (float32), participants /
# front / wide [npairs] (int32), masks: one bool array per pair, points: one [m][3] float32 array
# per pair (None for points=False)
Pose = collections.namedtuple("Pose", "R t participants front wide masks points")


def track_features(rows, offsets):
    """Buffer rows -> (set, feature): the set s with offsets[s] <= row < offsets[s + 1] and the
    row's index in it; two int arrays of rows' shape.  With the image offsets of a batch that is
    (image, feature)."""
    off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
    r = np.asarray(rows, np.int64)
    s = np.searchsorted(off, r, side="right") - 1
    if len(r) and (len(off) < 2 or s.min() < 0 or r.max() >= off[-1]):
        raise ValueError("a row lies outside the sets")
    return s.astype(np.int32), (r - off[s]).astype(np.int32)


class MatchOverflow(RuntimeError):
    """match_batch / match_images found more matches than `cap` (SGPU_ERANGE): .counts holds
    every pair's complete count, .matches the leading pairs that fit."""

    def __init__(self, counts, matches):
        super().__init__(f"{int(counts.sum())} matches exceed cap")
        self.counts = counts
        self.matches = matches


class SiftContext:
    """One HIP device context (sgpu_ctx)."""

    def __init__(self, device: int = 0, opts: SgpuOptions | None = None):
        self.opts = opts or default_options()
        self.device = device
        self._ctx = ctypes.c_void_p()
        rc = lib().sgpu_ctx_create(device, ctypes.byref(self.opts), ctypes.byref(self._ctx))
        if rc != SGPU_OK:
            raise RuntimeError(f"sgpu_ctx_create(device={device}) failed with {rc}: "
                               "no usable gfx950 device")
        self.batch = 0

    def close(self):
        if self._ctx:
            lib().sgpu_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != SGPU_OK:
            raise RuntimeError(f"{what} failed ({rc}): {lib().sgpu_last_error(self._ctx).decode()}")

    def set_options(self, opts: SgpuOptions):
        self.opts = opts
        self._check(lib().sgpu_ctx_set_options(self._ctx, ctypes.byref(opts)), "set_options")

    def reserve(self, n: int, w: int, h: int):
        """Allocate every buffer an extract of n u8 images of w x h needs (sgpu_reserve, the
        SiftGPU::AllocatePyramid entry point); drops the current batch and staged input."""
        self._check(lib().sgpu_reserve(self._ctx, n, w, h, w), "sgpu_reserve")
        self._staged = None
        self.batch = 0
        return self

    def pyramid_launches(self):
        """(kernel launches, level filters) of the last extract's Gaussian pyramid."""
        f = ctypes.c_int(0)
        n = lib().sgpu_last_pyramid_launches(self._ctx, ctypes.byref(f))
        if n < 0:
            raise RuntimeError("sgpu_last_pyramid_launches: no extract")
        return int(n), int(f.value)

    def pyramid_plan(self):
        """The launch list of the last extract's Gaussian pyramid (sgpu_debug_pyramid_plan), in
        issue order: a list of (kind, levels) with kind one of PLAN_KINDS and levels the (octave,
        level written) of each level filter the launch runs."""
        n = lib().sgpu_debug_pyramid_plan(self._ctx, None, 0)
        if n < 0:
            raise RuntimeError("sgpu_debug_pyramid_plan: no extract")
        out = np.zeros((n, 7), np.int32)
        self._check(min(0, lib().sgpu_debug_pyramid_plan(self._ctx, out.ctypes.data, out.size)),
                    "sgpu_debug_pyramid_plan")
        return [(PLAN_KINDS[int(e[0])], [(int(e[1 + 2 * j]), int(e[2 + 2 * j]))
                                         for j in range(3) if e[1 + 2 * j] >= 0]) for e in out]

    def set_stage_timing(self, on: bool):
        """Per-stage HIP events on/off (sgpu_set_stage_timing; the reference's _timingS)."""
        self._check(lib().sgpu_set_stage_timing(self._ctx, int(bool(on))), "sgpu_set_stage_timing")

    @staticmethod
    def alloc_count() -> int:
        """Device + pinned allocations the library has made so far (sgpu_debug_alloc_count)."""
        return int(lib().sgpu_debug_alloc_count())

    @staticmethod
    def _padded(images, stride, shape, dtype, channels=1):
        """A flat buffer of n images whose rows are `stride` elements apart (stride given), or a
        dense [n, h, w(, c)] array (stride None): (array, n, h, w, stride).  The library reads
        n * h * stride elements, so the flat buffer must hold them (the last row's padding too)."""
        if stride is None:
            a = np.ascontiguousarray(images, dtype)
            if a.ndim == (2 if channels == 1 else 3):
                a = a[None]
            if a.ndim != (3 if channels == 1 else 4):
                raise ValueError(f"images must be [n, h, w{'' if channels == 1 else ', c'}], got {a.shape}")
            n, h, w = a.shape[:3]
            if channels != 1 and a.shape[3] != channels:
                raise ValueError("channel count does not match the format")
            return a, n, h, w, w * channels
        if shape is None:
            raise ValueError("a row stride needs shape=(n, h, w)")
        n, h, w = (int(v) for v in shape)
        a = np.ascontiguousarray(images, dtype).reshape(-1)
        stride = int(stride)
        if stride < w * channels or a.size < n * h * stride:
            raise ValueError(f"{a.size} elements do not hold {n} x {h} rows {stride} apart "
                             f"of {w * channels}")
        return a, n, h, w, stride

    def stage(self, images: np.ndarray, stride=None, shape=None):
        """Upload a u8 batch [n, h, w] once; extract_staged() then starts from HBM.  With
        stride (bytes between rows): images is the flat buffer and shape = (n, h, w)."""
        a, n, h, w, stride = self._padded(images, stride, shape, np.uint8)
        self._check(lib().sgpu_stage_input(self._ctx, a.ctypes.data, n, w, h, stride), "stage")
        self._staged = (n, h, w, stride)
        return self

    def extract_staged(self):
        n, h, w, stride = self._staged
        self._check(lib().sgpu_extract(self._ctx, None, n, w, h, stride, SGPU_INPUT_STAGED),
                    "sgpu_extract(staged)")
        self.batch = n
        return self

    def extract(self, images: np.ndarray | int, shape=None, device_ptr=False, stride=None,
                dtype=None):
        """images: u8 or f32 [n, h, w] (or [h, w]) host array; or, with stride (elements between
        rows), the flat host buffer of shape=(n, h, w); or an int device pointer with
        shape=(n, h, w, stride) and dtype np.uint8 (default) / np.float32."""
        if device_ptr:
            n, h, w, stride = shape
            dt = np.dtype(np.uint8 if dtype is None else dtype)
        else:
            dt = np.dtype(np.asarray(images).dtype if dtype is None else dtype)
        if dt not in (np.dtype(np.uint8), np.dtype(np.float32)):
            raise TypeError(dt)
        fn = lib().sgpu_extract if dt == np.uint8 else lib().sgpu_extract_f32
        if device_ptr:
            rc = fn(self._ctx, ctypes.c_void_p(images), n, w, h, stride, SGPU_INPUT_DEVICE)
        else:
            a, n, h, w, stride = self._padded(images, stride, shape, dt)
            rc = fn(self._ctx, a.ctypes.data, n, w, h, stride, SGPU_INPUT_HOST)
        self._check(rc, "sgpu_extract")
        self.batch = n
        return self

    COLOR_FORMATS = {"rgb": 1, "bgr": 2, "rgba": 3, "bgra": 4}

    def extract_color(self, images: np.ndarray | int, fmt: str = "rgb", stride=None, shape=None,
                      device_ptr=False):
        """u8 color images [n, h, w, 3|4] (or [h, w, c]): luminance on the device with the
        reference's formula (GLTexImage.cpp:834-858), then the usual pipeline.  With stride (bytes
        between rows): images is the flat buffer of shape=(n, h, w); with device_ptr an int device
        pointer with shape=(n, h, w, stride)."""
        c = 3 if fmt in ("rgb", "bgr") else 4
        if device_ptr:
            n, h, w, stride = shape
            rc = lib().sgpu_extract_color(self._ctx, ctypes.c_void_p(images), n, w, h, stride,
                                          self.COLOR_FORMATS[fmt], SGPU_INPUT_DEVICE)
        else:
            a, n, h, w, stride = self._padded(images, stride, shape, np.uint8, c)
            rc = lib().sgpu_extract_color(self._ctx, a.ctypes.data, n, w, h, stride,
                                          self.COLOR_FORMATS[fmt], SGPU_INPUT_HOST)
        self._check(rc, "extract_color")
        self.batch = n

    def extract_stream(self, batches, keys=None, desc=None, cap=None, stride=None, shape=None):
        """Host-in / host-out extraction of a list of u8 batches [n, h, w] (sgpu_extract_stream:
        uploads and downloads overlap the kernels).  keys / desc: optional preallocated [cap, 4] /
        [cap, 128] float32 outputs (PinnedArray(...).array for overlapped copies).  With stride
        (bytes between rows): every batch is a flat buffer of shape=(n, h, w).  Returns
        (keys, desc, counts[total images]) trimmed to the features written."""
        if not len(batches):
            raise ValueError("no batches")
        if stride is None:
            bl = [np.ascontiguousarray(b) for b in batches]
            n, h, w = bl[0].shape
            if any(b.shape != (n, h, w) or b.dtype != np.uint8 for b in bl):
                raise ValueError("batches must be u8 arrays of one shape")
            stride = w
        else:
            if any(np.asarray(b).dtype != np.uint8 for b in batches):
                raise ValueError("batches must be u8 buffers")
            bl = [self._padded(b, stride, shape, np.uint8)[0] for b in batches]
            n, h, w = (int(v) for v in shape)
            stride = int(stride)
        want_desc = bool(self.opts.descriptors)

        def check_out(a, width, name):
            # the library's copies write cap rows: the array must hold them as C-ordered f32
            if (not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2 or
                    a.shape[1] != width or not a.flags.c_contiguous or not a.flags.writeable):
                raise ValueError(f"{name} must be a writable C-contiguous float32 [cap, {width}]")
        if keys is not None:
            check_out(keys, 4, "keys")
        if desc is not None:
            if not want_desc:
                raise ValueError("descriptors are disabled (-sd): pass desc=None")
            check_out(desc, 128, "desc")
        given = [len(a) for a in (keys, desc) if a is not None]
        if cap is None:
            cap = min(given) if given else 4096 * n * len(bl)
        cap = int(cap)
        if cap < 0 or any(cap > g for g in given):
            raise ValueError(f"cap {cap} exceeds an output array ({given})")
        if keys is None:
            keys = np.zeros((cap, 4), np.float32)
        if desc is None and want_desc:
            desc = np.zeros((cap, 128), np.float32)
        ptrs = (ctypes.c_void_p * len(bl))(*[b.ctypes.data for b in bl])
        counts = np.zeros(n * len(bl), np.int32)
        rc = lib().sgpu_extract_stream(self._ctx, ptrs, len(bl), n, w, h, stride, keys.ctypes.data,
                                       desc.ctypes.data if desc is not None else None, cap,
                                       counts.ctypes.data)
        self._check(rc, "sgpu_extract_stream")
        t = int(counts.sum())
        self.batch = 0
        return keys[:t], (desc[:t] if desc is not None else None), counts

    def extract_keypoints(self, keys: np.ndarray, has_orientation=True, image: int = 0):
        """Descriptors of caller-supplied keys [n, 4] (x, y, scale, orientation) on image
        `image` of the last extract (SiftGPU::RunSIFT(num, keys, keys_have_orientation)).
        has_orientation = -1: rectangles (x, y, width, height), the RECT description."""
        k = np.ascontiguousarray(keys, np.float32).reshape(-1, 4)
        ho = -1 if has_orientation == -1 else (1 if has_orientation else 0)
        self._check(lib().sgpu_extract_keypoints(self._ctx, image, k.ctypes.data, len(k), ho),
                    "sgpu_extract_keypoints")
        return self

    def count(self, image: int = 0) -> int:
        return lib().sgpu_feature_count(self._ctx, image)

    def total(self) -> int:
        return lib().sgpu_feature_total(self._ctx)

    def features(self, image: int = 0, descriptors: bool = True):
        n = self.count(image)
        keys = np.zeros((n, 4), np.float32)
        desc = np.zeros((n, 128), np.float32) if descriptors else None
        self._check(lib().sgpu_copy_features(self._ctx, image, keys.ctypes.data if n else None,
                                             desc.ctypes.data if (n and descriptors) else None),
                    "sgpu_copy_features")
        return keys, desc

    def set_host_output(self, keys, descriptors, capacity: int):
        """Register page-locked buffers (PinnedArray .array, [cap, 4] / [cap, 128] float32) that
        the next one-image extract fills from the GPU (sgpu_set_host_output)."""
        self._check(lib().sgpu_set_host_output(
            self._ctx, keys.ctypes.data if keys is not None else None,
            descriptors.ctypes.data if descriptors is not None else None, int(capacity)),
            "sgpu_set_host_output")

    def copy_features_into(self, keys, descriptors, image: int = 0):
        """sgpu_copy_features into caller arrays (e.g. the registered host output)."""
        self._check(lib().sgpu_copy_features(
            self._ctx, image, keys.ctypes.data if keys is not None else None,
            descriptors.ctypes.data if descriptors is not None else None), "sgpu_copy_features")

    def timing(self):
        t = np.zeros(10, np.float32)
        lib().sgpu_last_timing(self._ctx, t.ctypes.data, 10)
        return dict(zip(["upload", "pyramid", "detect", "orientation", "expand", "descriptor",
                         "download", "total", "match", "list"], t.tolist()))

    def match_shard_begin(self, d1_shard: np.ndarray, row_begin: int, d2: np.ndarray,
                          distmax=0.7, ratiomax=0.8, mbm=1):
        """Rows [row_begin, row_begin + len(d1_shard)) of set 1 against all of set 2
        (sgpu_match_shard_begin): (row decisions [ns], column state [n2][3])."""
        d1 = np.ascontiguousarray(d1_shard, np.uint8)
        d2 = np.ascontiguousarray(d2, np.uint8)
        ns, n2 = d1.shape[0], d2.shape[0]
        rows = np.zeros(max(ns, 1), np.int32)
        cols = np.zeros((max(n2, 1), 3), np.int32)
        self._check(lib().sgpu_match_shard_begin(self._ctx, d1.ctypes.data, ns, row_begin,
                                                 d2.ctypes.data, n2, distmax, ratiomax, mbm,
                                                 rows.ctypes.data, cols.ctypes.data,
                                                 SGPU_INPUT_HOST), "sgpu_match_shard_begin")
        return rows[:ns].copy(), cols[:n2].copy()

    def match_sharded(self, d1_shard: np.ndarray, row_begin: int, d2: np.ndarray,
                      distmax=0.7, ratiomax=0.8, mbm=1, max_match=None):
        """This rank's pairs of the sharded matcher; the column states travel by RCCL over the
        context's communicator (comm_init), or stay local without one (sgpu_match_sharded)."""
        d1 = np.ascontiguousarray(d1_shard, np.uint8)
        d2 = np.ascontiguousarray(d2, np.uint8)
        ns = d1.shape[0]
        max_match = ns if max_match is None else max_match
        out = np.zeros((max(max_match, 1), 2), np.int32)
        m = lib().sgpu_match_sharded(self._ctx, d1.ctypes.data, ns, row_begin, d2.ctypes.data,
                                     d2.shape[0], distmax, ratiomax, mbm, max_match,
                                     out.ctypes.data, SGPU_INPUT_HOST)
        if m < 0:
            self._check(m, "sgpu_match_sharded")
        return out[:m].copy()

    def match(self, d1: np.ndarray, d2: np.ndarray, distmax=0.7, ratiomax=0.8, mbm=1,
              max_match=None, device_ptrs=None):
        if device_ptrs is not None:
            p1, n1, p2, n2 = device_ptrs
            flags = SGPU_INPUT_DEVICE
        else:
            d1 = np.ascontiguousarray(d1, np.uint8)
            d2 = np.ascontiguousarray(d2, np.uint8)
            p1, n1, p2, n2 = d1.ctypes.data, d1.shape[0], d2.ctypes.data, d2.shape[0]
            flags = SGPU_INPUT_HOST
        max_match = n1 if max_match is None else max_match
        out = np.zeros((max(max_match, 1), 2), np.int32)
        m = lib().sgpu_match(self._ctx, ctypes.c_void_p(p1), n1, ctypes.c_void_p(p2), n2,
                             distmax, ratiomax, mbm, max_match, out.ctypes.data, flags)
        if m < 0:
            self._check(m, "sgpu_match")
        return out[:m]

    def quantize_gpu(self, desc: np.ndarray, device_ptrs=None):
        """Float descriptors [n, 128] -> u8 on the device, byte for byte sgpu.quantize().
        device_ptrs = (float descriptors, n, u8 output): int device pointers, written in place
        (SGPU_INPUT_DEVICE); returns None."""
        if device_ptrs is not None:
            src, n, dst = device_ptrs
            self._check(lib().sgpu_quantize_descriptors_gpu(
                self._ctx, ctypes.c_void_p(src), n, ctypes.c_void_p(dst), SGPU_INPUT_DEVICE),
                "sgpu_quantize_descriptors_gpu")
            return None
        d = np.ascontiguousarray(desc, np.float32).reshape(-1, 128)
        out = np.empty(d.shape, np.uint8)
        self._check(lib().sgpu_quantize_descriptors_gpu(self._ctx, d.ctypes.data, d.shape[0],
                                                        out.ctypes.data, SGPU_INPUT_HOST),
                    "sgpu_quantize_descriptors_gpu")
        return out

    def features_u8(self, image: int = 0) -> np.ndarray:
        """Image `image`'s descriptors of the last extract as u8 [n, 128], quantised on the
        device (sgpu_copy_features_u8)."""
        out = np.zeros((self.count(image), 128), np.uint8)
        self._check(lib().sgpu_copy_features_u8(self._ctx, image, out.ctypes.data if len(out) else None),
                    "sgpu_copy_features_u8")
        return out

    @staticmethod
    def _default_cap(first, sizes, limit):
        """The capacity that holds every pair's matches: min(rows of its first set, limit) summed
        over the pairs; 0 where an index lies outside the sets (the library refuses that list)."""
        first = np.asarray(first, np.int64).reshape(-1)
        ok = len(first) and limit > 0 and (first >= 0).all() and (first < len(sizes)).all()
        return int(np.minimum(np.asarray(sizes, np.int64)[first], limit).sum()) if ok else 0

    def _fitting(self, rc, what, out, counts, cap, verified=None):
        """One [m, 2] array per pair of the matches a call brought down: the pairs that fit cap form
        a prefix.  SGPU_ERANGE raises MatchOverflow with them (and .verified, where given)."""
        if rc < 0 and rc != SGPU_ERANGE:
            self._check(rc, what)
        offs = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        res = [out[offs[p]:offs[p + 1]].copy() for p in range(len(counts)) if offs[p + 1] <= cap]
        if rc == SGPU_ERANGE:
            e = MatchOverflow(counts.copy(), res)
            if verified is not None:
                e.verified = verified
            raise e
        return res

    def _pair_results(self, call, pairs, sizes, max_match, cap):
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        npairs = len(pr)
        if max_match is None:
            max_match = int(max(sizes)) if len(sizes) else 0
        cap = self._default_cap(pr[:, 0], sizes, max_match) if cap is None else int(cap)
        out = np.zeros((max(cap, 1), 2), np.int32)
        counts = np.zeros(max(npairs, 1), np.int32)
        rc = call(pr, npairs, int(max_match), out, cap, counts)
        return self._fitting(rc, "match batch", out, counts[:npairs], cap)

    def match_batch(self, desc_u8: np.ndarray, offsets, pairs, distmax=0.7, ratiomax=0.8, mbm=1,
                    max_match=None, cap=None):
        """Many set pairs of one u8 descriptor buffer in one call (sgpu_match_batch): set s =
        rows [offsets[s], offsets[s + 1]), pairs [(a, b), ...].  Returns one [m, 2] int32 array
        per pair, each what match(set a, set b) returns.  max_match: per pair (default: no
        limit); cap: total capacity (default: enough for every pair); more matches than cap raise
        MatchOverflow."""
        d = np.ascontiguousarray(desc_u8, np.uint8).reshape(-1, 128)
        off = np.ascontiguousarray(offsets, np.int64)
        nsets = len(off) - 1
        if nsets < 0 or (nsets >= 0 and len(off) and off[-1] > len(d)):
            raise ValueError("offsets do not fit the descriptor buffer")
        sizes = np.diff(off)

        def call(pr, npairs, mm, out, cp, counts):
            return lib().sgpu_match_batch(self._ctx, d.ctypes.data if len(d) else None,
                                          off.ctypes.data, nsets, pr.ctypes.data if npairs else None,
                                          npairs, distmax, ratiomax, mbm, mm, out.ctypes.data, cp,
                                          counts.ctypes.data, SGPU_INPUT_HOST)
        return self._pair_results(call, pairs, sizes, max_match, cap)

    def match_images(self, pairs, distmax=0.7, ratiomax=0.8, mbm=1, max_match=None, cap=None):
        """Image pairs [(a, b), ...] of the last extract matched on the device
        (sgpu_match_images): the descriptors are quantised in HBM and never leave it.  Returns
        one [m, 2] int32 array per pair."""
        sizes = np.array([self.count(i) for i in range(self.batch)], np.int64)

        def call(pr, npairs, mm, out, cp, counts):
            return lib().sgpu_match_images(self._ctx, pr.ctypes.data if npairs else None, npairs,
                                           distmax, ratiomax, mbm, mm, out.ctypes.data, cp,
                                           counts.ctypes.data)
        return self._pair_results(call, pairs, sizes, max_match, cap)

    @staticmethod
    def _pair_matrices(M, npairs, name):
        """H / F of a guided pair list: [npairs][3][3] (or [npairs][9]) float32, or None."""
        if M is None:
            return None
        m = np.ascontiguousarray(M, np.float32)
        if m.size != 9 * npairs or m.ndim < 2 or m.shape[0] != npairs:
            raise ValueError(f"{name} must be [npairs][3][3] ({npairs} pairs), got {m.shape}")
        return m.reshape(npairs, 9)

    def match_batch_guided(self, desc_u8: np.ndarray, loc: np.ndarray, offsets, pairs, H=None,
                           F=None, distmax=0.7, ratiomax=0.8, hdistmax=32.0, fdistmax=16.0, mbm=1,
                           max_match=None, cap=None):
        """Guided matching of many set pairs in one call (sgpu_match_batch_guided): the sets of
        match_batch with their locations loc [rows][2] (x, y), and per pair p its own H[p] / F[p]
        ([npairs][3][3], or None for all pairs).  Returns one [m, 2] int32 array per pair, each
        what match_guided(set a, set b, loc a, loc b, H[p], F[p]) returns."""
        d = np.ascontiguousarray(desc_u8, np.uint8).reshape(-1, 128)
        lc = np.ascontiguousarray(loc, np.float32)
        if lc.ndim != 2 or lc.shape != (len(d), 2):
            raise ValueError(f"locations must be [rows][2] for {len(d)} rows, got {lc.shape}")
        off = np.ascontiguousarray(offsets, np.int64)
        nsets = len(off) - 1
        if nsets < 0 or (nsets >= 0 and len(off) and off[-1] > len(d)):
            raise ValueError("offsets do not fit the descriptor buffer")
        sizes = np.diff(off)
        npr = len(np.asarray(pairs, np.int32).reshape(-1, 2))
        hm = self._pair_matrices(H, npr, "H")
        fm = self._pair_matrices(F, npr, "F")

        def call(pr, npairs, mm, out, cp, counts):
            return lib().sgpu_match_batch_guided(
                self._ctx, d.ctypes.data if len(d) else None, lc.ctypes.data if len(lc) else None,
                off.ctypes.data, nsets, pr.ctypes.data if npairs else None, npairs,
                None if hm is None else hm.ctypes.data, None if fm is None else fm.ctypes.data,
                distmax, ratiomax, hdistmax, fdistmax, mbm, mm, out.ctypes.data, cp,
                counts.ctypes.data, SGPU_INPUT_HOST)
        return self._pair_results(call, pairs, sizes, max_match, cap)

    def match_images_guided(self, pairs, H=None, F=None, distmax=0.7, ratiomax=0.8, hdistmax=32.0,
                            fdistmax=16.0, mbm=1, max_match=None, cap=None):
        """Image pairs of the last extract matched under per-pair geometry on the device
        (sgpu_match_images_guided): descriptors as match_images, locations = x, y of the batch's
        device keys; neither leaves HBM.  H / F: [npairs][3][3] or None."""
        npr = len(np.asarray(pairs, np.int32).reshape(-1, 2))
        hm = self._pair_matrices(H, npr, "H")
        fm = self._pair_matrices(F, npr, "F")
        sizes = np.array([self.count(i) for i in range(self.batch)], np.int64)

        def call(pr, npairs, mm, out, cp, counts):
            return lib().sgpu_match_images_guided(
                self._ctx, pr.ctypes.data if npairs else None, npairs,
                None if hm is None else hm.ctypes.data, None if fm is None else fm.ctypes.data,
                distmax, ratiomax, hdistmax, fdistmax, mbm, mm, out.ctypes.data, cp,
                counts.ctypes.data)
        return self._pair_results(call, pairs, sizes, max_match, cap)

    MODELS = {"H": 0, "F": 1}   # SGPU_MODEL_HOMOGRAPHY / SGPU_MODEL_FUNDAMENTAL

    def _estimate(self, call, pairs, matches, model, threshold, iterations, seed, rounds=None):
        """Common part of estimate_batch / estimate_images and their refined forms: the pair list
        and the per-pair [m, 2] match arrays go down concatenated; (models [npairs][3][3] float32,
        inliers [npairs] int32, masks: one bool array per pair) come back, and with rounds (the
        refined forms: call takes the round budget and the output array last) the accepted rounds
        [npairs] int32 as a fourth."""
        if model not in self.MODELS:
            raise ValueError(f'model must be "H" or "F", got {model!r}')
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        npairs = len(pr)
        if len(matches) != npairs:
            raise ValueError(f"{npairs} pairs but {len(matches)} match arrays")
        ms = [np.ascontiguousarray(m, np.int32).reshape(-1, 2) for m in matches]
        counts = np.array([len(m) for m in ms], np.int32).reshape(npairs)
        cat = (np.concatenate(ms) if npairs else np.zeros((0, 2), np.int32)).astype(np.int32)
        cat = np.ascontiguousarray(cat)
        total = len(cat)
        models = np.zeros((max(npairs, 1), 9), np.float32)
        inliers = np.zeros(max(npairs, 1), np.int32)
        mask = np.zeros(max(total, 1), np.uint8)
        done = np.zeros(max(npairs, 1), np.int32)
        extra = () if rounds is None else (int(rounds), done.ctypes.data)
        rc = call(pr.ctypes.data if npairs else None, npairs, cat.ctypes.data if total else None,
                  counts.ctypes.data if npairs else None, self.MODELS[model], float(threshold),
                  int(iterations), int(seed) & 0xFFFFFFFF, models.ctypes.data, inliers.ctypes.data,
                  mask.ctypes.data, *extra)
        self._check(rc, "estimate")
        offs = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        masks = [mask[offs[p]:offs[p + 1]].astype(bool) for p in range(npairs)]
        out = (models[:npairs].reshape(npairs, 3, 3).copy(), inliers[:npairs].copy(), masks)
        return out if rounds is None else out + (done[:npairs].copy(),)

    def estimate_batch(self, loc: np.ndarray, offsets, pairs, matches, model="H", threshold=2.0,
                       iterations=512, seed=0, device_ptr=None):
        """One H or F per set pair from its matches (sgpu_estimate_batch): loc [rows][2] (x, y) of
        the sets of match_batch, pairs [(a, b), ...], matches = the list of [m, 2] arrays that
        match_batch returned for them.  model "H": |H x1 - x2| < threshold in both coordinates;
        "F": Sampson error < threshold (squared pixels), no rank-2 enforcement.  Returns (models
        [npairs][3][3] float32 at unit Frobenius norm, ready for match_batch_guided; inlier counts
        [npairs]; one bool mask per pair).  A pair without a model has zeros.  device_ptr: the
        int device address of the locations, read in place (SGPU_INPUT_DEVICE; loc is ignored)."""
        off, nsets, lc, ptr, flags = self._estimate_sets(loc, offsets, device_ptr)

        def call(pr, npairs, cat, counts, mdl, thr, it, sd, models, inliers, mask):
            return lib().sgpu_estimate_batch(self._ctx, ptr, off.ctypes.data, nsets, pr, npairs, cat,
                                             counts, mdl, thr, it, sd, models, inliers, mask, flags)
        return self._estimate(call, pairs, matches, model, threshold, iterations, seed)

    @staticmethod
    def _estimate_sets(loc, offsets, device_ptr):
        """The set arguments of estimate_batch: (offsets int64, nsets, the host array kept alive,
        the locations' pointer, the input flag)."""
        off = np.ascontiguousarray(offsets, np.int64)
        nsets = len(off) - 1
        if device_ptr is not None:
            return off, nsets, None, ctypes.c_void_p(device_ptr), SGPU_INPUT_DEVICE
        lc = np.ascontiguousarray(loc, np.float32)
        if lc.ndim != 2 or lc.shape[1] != 2 or nsets < 0 or (len(off) and off[-1] > len(lc)):
            raise ValueError(f"locations must be [rows][2] covering the offsets, got {lc.shape}")
        return off, nsets, lc, (lc.ctypes.data if len(lc) else None), SGPU_INPUT_HOST

    def estimate_batch_refined(self, loc: np.ndarray, offsets, pairs, matches, model="H",
                               threshold=2.0, iterations=512, seed=0, rounds=3, device_ptr=None):
        """estimate_batch, then up to `rounds` (0 .. 16) least-squares refits of every pair's model
        on its own inliers, on the device (sgpu_estimate_batch_refined): a refit that would lose
        an inlier is rejected, so no count falls below estimate_batch's, and every mask is still
        the guided test of its returned matrix.  Returns (models, inliers, masks, rounds): the
        last = the accepted rounds of every pair, int32 [npairs]."""
        off, nsets, lc, ptr, flags = self._estimate_sets(loc, offsets, device_ptr)

        def call(pr, npairs, cat, counts, mdl, thr, it, sd, models, inliers, mask, budget, done):
            return lib().sgpu_estimate_batch_refined(self._ctx, ptr, off.ctypes.data, nsets, pr,
                                                     npairs, cat, counts, mdl, thr, it, sd, budget,
                                                     models, inliers, mask, done, flags)
        return self._estimate(call, pairs, matches, model, threshold, iterations, seed, rounds)

    def estimate_images_refined(self, pairs, matches, model="H", threshold=2.0, iterations=512,
                                seed=0, rounds=3):
        """estimate_batch_refined over the last extract (sgpu_estimate_images_refined)."""
        def call(pr, npairs, cat, counts, mdl, thr, it, sd, models, inliers, mask, budget, done):
            return lib().sgpu_estimate_images_refined(self._ctx, pr, npairs, cat, counts, mdl, thr,
                                                      it, sd, budget, models, inliers, mask, done)
        return self._estimate(call, pairs, matches, model, threshold, iterations, seed, rounds)

    def estimate_images(self, pairs, matches, model="H", threshold=2.0, iterations=512, seed=0):
        """estimate_batch over the last extract (sgpu_estimate_images): pairs of its images, matches
        as match_images returned them; the locations are the batch's device keys and stay in HBM."""
        def call(pr, npairs, cat, counts, mdl, thr, it, sd, models, inliers, mask):
            return lib().sgpu_estimate_images(self._ctx, pr, npairs, cat, counts, mdl, thr, it, sd,
                                              models, inliers, mask)
        return self._estimate(call, pairs, matches, model, threshold, iterations, seed)

    @staticmethod
    def verify_params(**params) -> SgpuVerifyParams:
        """sgpu_default_verify_params with the given fields of sgpu_verify_params replaced."""
        vp = SgpuVerifyParams()
        lib().sgpu_default_verify_params(ctypes.byref(vp))
        names = {f[0] for f in SgpuVerifyParams._fields_}
        for k, v in params.items():
            if k not in names:
                raise TypeError(f"unknown verify parameter {k!r}")
            setattr(vp, k, int(v) & 0xFFFFFFFF if k == "seed" else v)
        return vp

    def _verify(self, call, pairs, sizes, H, F, cap, params):
        """Common part of verify_batch / verify_images: call(pairs pointer, npairs, params, the
        five model outputs' pointers, out, cap, counts) -> the C return value."""
        if not H and not F:
            raise ValueError("verify needs a model: H, F or both (match_batch matches without one)")
        vp = self.verify_params(**params)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        npairs = len(pr)
        cap = self._default_cap(pr[:, 0], sizes, vp.max_match) if cap is None else int(cap)
        out = np.zeros((max(cap, 1), 2), np.int32)
        counts = np.zeros(max(npairs, 1), np.int32)
        putative = np.zeros(max(npairs, 1), np.int32)
        models = [np.zeros((max(npairs, 1), 9), np.float32) if want else None for want in (H, F)]
        inliers = [np.zeros(max(npairs, 1), np.int32) if want else None for want in (H, F)]
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = call(pr.ctypes.data if npairs else None, npairs, ctypes.byref(vp), ptr(models[0]),
                  ptr(inliers[0]), ptr(models[1]), ptr(inliers[1]), putative.ctypes.data,
                  out.ctypes.data, cap, counts.ctypes.data)
        ms = [None if m is None else m[:npairs].reshape(npairs, 3, 3).copy() for m in models]
        ins = [None if i is None else i[:npairs].copy() for i in inliers]
        rest = (ms[0], ins[0], ms[1], ins[1], putative[:npairs].copy())
        return (self._fitting(rc, "verify", out, counts[:npairs], cap, rest),) + rest

    def verify_batch(self, desc_u8, loc, offsets, pairs, H=True, F=False, cap=None,
                     device_ptrs=None, **params):
        """Verified matches of many set pairs in one call (sgpu_verify_batch): match_batch, then
        estimate_batch_refined for H and / or F, then match_batch_guided under those models, all on
        the device -- the bits of that chain.  desc_u8 [rows][128], loc [rows][2], offsets and
        pairs as match_batch_guided; params: fields of sgpu_verify_params (verify_params()).
        Returns (one [m, 2] int32 array per pair, H [npairs][3][3], inliers_H [npairs], F,
        inliers_F, putative counts [npairs]), None for a model not asked for; more verified matches
        than cap raise MatchOverflow (its .verified = the other five).  device_ptrs = (descriptors,
        locations): int device addresses read in place (SGPU_INPUT_DEVICE; desc_u8, loc ignored)."""
        off = np.ascontiguousarray(offsets, np.int64)
        nsets = len(off) - 1
        if device_ptrs is not None:
            dp, lp = (ctypes.c_void_p(a) for a in device_ptrs)
            flags = SGPU_INPUT_DEVICE
            if nsets < 0:
                raise ValueError("offsets must hold at least one entry")
        else:
            d = np.ascontiguousarray(desc_u8, np.uint8).reshape(-1, 128)
            lc = np.ascontiguousarray(loc, np.float32)
            if lc.ndim != 2 or lc.shape != (len(d), 2):
                raise ValueError(f"locations must be [rows][2] for {len(d)} rows, got {lc.shape}")
            if nsets < 0 or (len(off) and off[-1] > len(d)):
                raise ValueError("offsets do not fit the descriptor buffer")
            dp, lp = (d.ctypes.data if len(d) else None), (lc.ctypes.data if len(lc) else None)
            flags = SGPU_INPUT_HOST

        def call(pr, npairs, vp, *outs):
            return lib().sgpu_verify_batch(self._ctx, dp, lp, off.ctypes.data, nsets, pr, npairs, vp,
                                           *outs, flags)
        return self._verify(call, pairs, np.diff(off), H, F, cap, params)

    def verify_images(self, pairs, H=True, F=False, cap=None, **params):
        """verify_batch over the last extract (sgpu_verify_images): descriptors and locations as
        match_images_guided takes them; nothing of them leaves HBM."""
        if not H and not F:
            raise ValueError("verify needs a model: H, F or both (match_images matches without one)")
        sizes = np.array([self.count(i) for i in range(self.batch)], np.int64)

        def call(pr, npairs, vp, *outs):
            return lib().sgpu_verify_images(self._ctx, pr, npairs, vp, *outs)
        return self._verify(call, pairs, sizes, H, F, cap, params)

    def verify_time(self) -> float:
        """Device milliseconds of the last verify_batch / verify_images (sgpu_last_timing's
        times[13]); timing() keeps the slots it has always returned."""
        t = np.zeros(14, np.float32)
        lib().sgpu_last_timing(self._ctx, t.ctypes.data, 14)
        return float(t[13])

    # ---- preemptive matching (sgpu_select_top_scale_*, sgpu_prematch_*)
    @staticmethod
    def _set_offsets(offsets):
        off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        if len(off) < 1:
            raise ValueError("offsets must hold at least one entry")
        return off, len(off) - 1

    @staticmethod
    def _scales(scale, off, stride):
        """The host scales of select_top_scale / prematch_batch: a flat float32 buffer in which
        row r's scale is element r * stride."""
        sc = np.ascontiguousarray(scale, np.float32).reshape(-1)
        stride = int(stride)
        rows = int(off[-1])
        if stride < 1 or (rows > 0 and len(sc) < (rows - 1) * stride + 1):
            raise ValueError(f"{len(sc)} floats do not hold {rows} scales {stride} apart")
        return sc, stride

    @staticmethod
    def _split(flat, offs):
        return [flat[offs[s]:offs[s + 1]].copy() for s in range(len(offs) - 1)]

    def select_top_scale(self, scale, offsets, top, stride=1, device_ptr=None):
        """Each set's min(n, top) largest-scale rows (sgpu_select_top_scale_batch; the rule of
        csrc/sift_select.h: equal scales resolve to the lower row): one ascending int32 array of
        set-local row indices per set.  scale: flat float32 buffer, row r's scale at r * stride;
        offsets as match_batch.  device_ptr: the int device address of the scales, read in place
        (SGPU_INPUT_DEVICE; scale is ignored)."""
        off, nsets = self._set_offsets(offsets)
        if device_ptr is not None:
            ptr, flags, stride = ctypes.c_void_p(device_ptr), SGPU_INPUT_DEVICE, int(stride)
        else:
            sc, stride = self._scales(scale, off, stride)
            ptr, flags = (sc.ctypes.data if len(sc) else None), SGPU_INPUT_HOST
        sizes = np.diff(off)
        cap = int(np.minimum(sizes, max(int(top), 0)).clip(0).sum()) if (sizes >= 0).all() else 0
        index = np.zeros(max(cap, 1), np.int32)
        sub = np.zeros(nsets + 1, np.int64)
        self._check(lib().sgpu_select_top_scale_batch(self._ctx, ptr, stride, off.ctypes.data, nsets,
                                                      int(top), index.ctypes.data, sub.ctypes.data,
                                                      flags), "sgpu_select_top_scale_batch")
        return self._split(index, sub)

    def select_top_scale_images(self, top):
        """select_top_scale over the last extract (sgpu_select_top_scale_images): the scales are
        column 2 of the batch's device keys."""
        cap = sum(min(self.count(i), max(int(top), 0)) for i in range(self.batch))
        index = np.zeros(max(cap, 1), np.int32)
        sub = np.zeros(self.batch + 1, np.int64)
        self._check(lib().sgpu_select_top_scale_images(self._ctx, int(top), index.ctypes.data,
                                                       sub.ctypes.data), "sgpu_select_top_scale_images")
        return self._split(index, sub)

    def _prematch(self, call, pairs, sizes, top, matches, cap):
        """Common part of prematch_batch / prematch_images: call(pairs pointer or None, npairs,
        counts, out or None, cap) -> the C return value."""
        nsets, top = len(sizes), int(top)
        if pairs is None:   # all pairs a < b: the library builds the list
            a, b = np.triu_indices(nsets, 1)
            first, npairs, ptr = a, len(a), None
        else:
            pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
            npairs = len(pr)
            first = pr[:, 0]
            # (an empty explicit list is not the all-pairs request: never a null pointer)
            keep = pr if npairs else np.zeros((1, 2), np.int32)
            ptr = keep.ctypes.data
        counts = np.zeros(max(npairs, 1), np.int32)
        out = None
        if matches:
            cap = self._default_cap(first, sizes, top) if cap is None else int(cap)
            out = np.zeros((max(cap, 1), 2), np.int32)
        rc = call(ptr, npairs, counts.ctypes.data, None if out is None else out.ctypes.data,
                  cap if matches else 0)
        counts = counts[:npairs]
        if not matches:
            if rc < 0 and rc != SGPU_ERANGE:
                self._check(rc, "prematch")
            return counts.copy(), None
        return counts.copy(), self._fitting(rc, "prematch", out, counts, cap)

    def prematch_batch(self, desc_u8, scale, offsets, pairs=None, top=100, distmax=0.7, ratiomax=0.8,
                       mbm=1, matches=True, cap=None, stride=1, device_ptrs=None):
        """Preemptive matching (sgpu_prematch_batch): every set's `top` largest-scale rows are
        selected and gathered on the device and the pairs matched on those subsets alone -- the bits
        of match_batch on the gathered subsets with max_match = top, each match reported in the
        sets' own row indices.  desc_u8, offsets, pairs as match_batch (pairs=None: all pairs
        a < b in lexicographic order); scale, stride as select_top_scale.  Returns (counts [npairs]
        int32, one [m, 2] int32 array per pair, or None with matches=False: counts only, nothing
        else comes down).  More matches than cap raise MatchOverflow.  device_ptrs = (descriptors,
        scales): int device addresses read in place (SGPU_INPUT_DEVICE)."""
        off, nsets = self._set_offsets(offsets)
        if device_ptrs is not None:
            dp, sp = (ctypes.c_void_p(a) for a in device_ptrs)
            flags, stride = SGPU_INPUT_DEVICE, int(stride)
        else:
            d = np.ascontiguousarray(desc_u8, np.uint8).reshape(-1, 128)
            if off[-1] > len(d):
                raise ValueError("offsets do not fit the descriptor buffer")
            sc, stride = self._scales(scale, off, stride)
            dp, sp = (d.ctypes.data if len(d) else None), (sc.ctypes.data if len(sc) else None)
            flags = SGPU_INPUT_HOST

        def call(pr, npairs, counts, out, cp):
            return lib().sgpu_prematch_batch(self._ctx, dp, sp, stride, off.ctypes.data, nsets, pr,
                                             npairs, int(top), distmax, ratiomax, mbm, counts, out,
                                             cp, flags)
        return self._prematch(call, pairs, np.diff(off), top, matches, cap)

    def prematch_images(self, pairs=None, top=100, distmax=0.7, ratiomax=0.8, mbm=1, matches=True,
                        cap=None):
        """prematch_batch over the last extract (sgpu_prematch_images): scales and descriptors are
        the batch's own device buffers; pairs=None: all image pairs a < b."""
        sizes = np.array([self.count(i) for i in range(self.batch)], np.int64)

        def call(pr, npairs, counts, out, cp):
            return lib().sgpu_prematch_images(self._ctx, pr, npairs, int(top), distmax, ratiomax, mbm,
                                              counts, out, cp)
        return self._prematch(call, pairs, sizes, top, matches, cap)

    def candidate_pairs(self, top=100, min_matches=4, distmax=0.7, ratiomax=0.8, mbm=1):
        """The image pairs a < b of the last extract worth matching in full: those with at least
        min_matches matches among their `top` largest-scale features (prematch_images over all
        pairs, counts only; the threshold is applied here).  Returns (pairs [k][2] int32, their
        counts [k] int32), in lexicographic order."""
        counts, _ = self.prematch_images(None, top, distmax, ratiomax, mbm, matches=False)
        a, b = np.triu_indices(self.batch, 1)
        keep = counts >= int(min_matches)
        return np.stack([a[keep], b[keep]], axis=1).astype(np.int32).reshape(-1, 2), counts[keep]

    def prematch_time(self) -> float:
        """Device milliseconds of the last prematch_batch / prematch_images (sgpu_last_timing's
        times[14])."""
        t = np.zeros(15, np.float32)
        lib().sgpu_last_timing(self._ctx, t.ctypes.data, 15)
        return float(t[14])

    # ---- feature tracks (sgpu_tracks_*)
    @staticmethod
    def _track_inputs(pairs, matches, min_length):
        """The pair list and its per-pair [m, 2] matches as the C arrays: pairs [npairs][2],
        the concatenated matches [total][2], counts [npairs]."""
        pr = np.ascontiguousarray(pairs, np.int32)
        if pr.size and (pr.ndim != 2 or pr.shape[1] != 2):
            raise ValueError(f"pairs must be [npairs][2], got {pr.shape}")
        pr = pr.reshape(-1, 2)
        ms = [np.ascontiguousarray(m, np.int32) for m in matches]
        if len(ms) != len(pr):
            raise ValueError(f"{len(ms)} match lists for {len(pr)} pairs")
        for m in ms:
            if m.size and (m.ndim != 2 or m.shape[1] != 2):
                raise ValueError(f"a pair's matches must be [m][2], got {m.shape}")
        if int(min_length) < 2:
            raise ValueError("min_length < 2")
        counts = np.array([m.size // 2 for m in ms], np.int32)
        flat = np.concatenate([m.reshape(-1, 2) for m in ms] + [np.zeros((0, 2), np.int32)])
        return pr, np.ascontiguousarray(flat, np.int32), counts

    def _tracks(self, call, rows, pairs, matches, min_length):
        pr, flat, counts = self._track_inputs(pairs, matches, min_length)
        track = np.zeros(max(rows, 1), np.int32)
        offs = np.zeros(rows // 2 + 1, np.int64)
        out = np.zeros(max(rows, 1), np.int32)
        stats = np.zeros(4, np.int64)
        ptr = lambda a: a.ctypes.data if a.size else None
        T = call(ptr(pr), len(pr), ptr(flat), ptr(counts), int(min_length), track.ctypes.data,
                 offs.ctypes.data, out.ctypes.data, stats.ctypes.data)
        if T < 0:
            self._check(T, "tracks")
        return Tracks(track[:rows].copy(), offs[:T + 1].copy(), out[:offs[T]].copy(), stats)

    def tracks_batch(self, offsets, pairs, matches, min_length=2):
        """Feature tracks of a pair list's matches (sgpu_tracks_batch; the rule of
        csrc/sift_tracks.h): offsets and pairs as match_batch took them, matches the per-pair list
        match_batch / match_batch_guided / verify_batch returned.  A track is a connected component
        of the match graph with at least min_length rows and at most one row per set; tracks are
        numbered in ascending order of their smallest row.  Returns Tracks(track_of_row, offsets,
        rows, stats); track_features(rows, offsets) gives (set, feature)."""
        off, nsets = self._set_offsets(offsets)
        if (np.diff(off) < 0).any() or off[0] < 0:
            raise ValueError("offsets must be non-negative and non-decreasing")

        def call(pr, npairs, *rest):
            return lib().sgpu_tracks_batch(self._ctx, off.ctypes.data, nsets, pr, npairs, *rest)
        return self._tracks(call, int(off[-1]), pairs, matches, min_length)

    def tracks_images(self, pairs, matches, min_length=2):
        """tracks_batch over the last extract (sgpu_tracks_images): the sets are its images, pairs
        and matches what match_images / verify_images took and returned.  track_features(rows,
        image offsets) gives (image, feature)."""
        rows = sum(self.count(i) for i in range(self.batch))

        def call(pr, npairs, *rest):
            return lib().sgpu_tracks_images(self._ctx, pr, npairs, *rest)
        return self._tracks(call, rows, pairs, matches, min_length)

    def tracks_time(self) -> float:
        """Device milliseconds of the last tracks_batch / tracks_images (sgpu_last_timing's
        times[15])."""
        t = np.zeros(16, np.float32)
        lib().sgpu_last_timing(self._ctx, t.ctypes.data, 16)
        return float(t[15])

    # ---- relative pose of verified pairs (sgpu_pose_*)
    DEFAULT_MIN_ANGLE = float(np.deg2rad(2.0))

    @staticmethod
    def _pose_inputs(pairs, matches, F, K, nsets, threshold, min_angle):
        """The pair list, its per-pair [m, 2] matches, the pairs' F and the sets' intrinsics as the
        C arrays; every shape error is a ValueError here, before any C call."""
        pr = np.ascontiguousarray(pairs, np.int32)
        if pr.size and (pr.ndim != 2 or pr.shape[1] != 2):
            raise ValueError(f"pairs must be [npairs][2], got {pr.shape}")
        pr = pr.reshape(-1, 2)
        npairs = len(pr)
        if len(matches) != npairs:
            raise ValueError(f"{npairs} pairs but {len(matches)} match arrays")
        ms = [np.ascontiguousarray(m, np.int32) for m in matches]
        for m in ms:
            if m.size and (m.ndim != 2 or m.shape[1] != 2):
                raise ValueError(f"a pair's matches must be [m][2], got {m.shape}")
        fm = np.ascontiguousarray(F, np.float32)
        if fm.size != 9 * npairs or (npairs and fm.shape not in ((npairs, 3, 3), (npairs, 9))):
            raise ValueError(f"F must be [{npairs}][3][3], got {fm.shape}")
        km = np.ascontiguousarray(K, np.float32)
        if km.ndim != 2 or km.shape[1] != 4 or (nsets is not None and len(km) != nsets):
            raise ValueError(f"K must be [sets][4] (fx, fy, cx, cy), got {km.shape}")
        if not (float(threshold) >= 0 and np.isfinite(threshold)):
            raise ValueError("threshold negative or not finite")
        if not 0 <= float(min_angle) <= np.pi / 2 + 1e-7:
            raise ValueError("min_angle outside [0, pi/2]")
        counts = np.array([m.size // 2 for m in ms], np.int32)
        flat = np.concatenate([m.reshape(-1, 2) for m in ms] + [np.zeros((0, 2), np.int32)])
        return pr, np.ascontiguousarray(flat, np.int32), counts, fm.reshape(-1, 9), km

    def _pose(self, call, inputs, threshold, min_angle, points):
        pr, flat, counts, fm, km = inputs
        npairs, total = len(pr), len(flat)
        R = np.zeros((max(npairs, 1), 9), np.float32)
        t = np.zeros((max(npairs, 1), 3), np.float32)
        oc = np.zeros((max(npairs, 1), 3), np.int32)
        mask = np.zeros(max(total, 1), np.uint8)
        pts = np.zeros((max(total, 1), 3), np.float32) if points else None
        ptr = lambda a: a.ctypes.data if a.size else None
        rc = call(ptr(km), ptr(pr), npairs, ptr(flat), ptr(counts), ptr(fm), float(threshold),
                  float(min_angle), R.ctypes.data, t.ctypes.data, oc.ctypes.data, mask.ctypes.data,
                  pts.ctypes.data if points else None)
        self._check(rc, "pose")
        offs = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        masks = [mask[offs[p]:offs[p + 1]].astype(bool) for p in range(npairs)]
        plist = [pts[offs[p]:offs[p + 1]].copy() for p in range(npairs)] if points else None
        return Pose(R[:npairs].reshape(npairs, 3, 3).copy(), t[:npairs].copy(), oc[:npairs, 0].copy(),
                    oc[:npairs, 1].copy(), oc[:npairs, 2].copy(), masks, plist)

    def pose_batch(self, loc: np.ndarray, offsets, pairs, matches, F, K, threshold=4.0,
                   min_angle=DEFAULT_MIN_ANGLE, points=True, device_ptr=None):
        """Relative pose and triangulation of every pair (sgpu_pose_batch; the rule of
        csrc/sift_pose.h): loc, offsets, pairs and matches as estimate_batch took them, F
        [npairs][3][3] as estimate_batch / verify_batch returned it, K [sets][4] = (fx, fy, cx, cy).
        A match participates when its Sampson error under F is below threshold; the pair's E is
        decomposed, and the candidate (R, t) with the most participants in front of both cameras
        wins.  Returns Pose(R, t, participants, front, wide, masks, points): x_cam2 = R x_cam1 + t
        with |t| = 1; wide counts the in-front matches whose rays meet at min_angle (radians) or
        more; masks[p] marks the in-front participants, points[p] their X in the first camera's
        frame (zeros elsewhere; None with points=False).  A pair without a pose has zeros."""
        off, nsets, lc, ptr, flags = self._estimate_sets(loc, offsets, device_ptr)
        inputs = self._pose_inputs(pairs, matches, F, K, nsets, threshold, min_angle)

        def call(km, pr, npairs, *rest):
            return lib().sgpu_pose_batch(self._ctx, ptr, off.ctypes.data, nsets, km, pr, npairs,
                                         *rest, flags)
        return self._pose(call, inputs, threshold, min_angle, points)

    def pose_images(self, pairs, matches, F, K, threshold=4.0, min_angle=DEFAULT_MIN_ANGLE,
                    points=True):
        """pose_batch over the last extract (sgpu_pose_images): the sets are its images, K
        [batch][4]; the locations are the batch's device keys and stay in HBM."""
        batch = getattr(self, "batch", 0) or None   # without a batch the call itself refuses
        inputs = self._pose_inputs(pairs, matches, F, K, batch, threshold, min_angle)

        def call(km, pr, npairs, *rest):
            return lib().sgpu_pose_images(self._ctx, km, pr, npairs, *rest)
        return self._pose(call, inputs, threshold, min_angle, points)

    def pose_time(self) -> float:
        """Device milliseconds of the last pose_batch / pose_images (sgpu_last_timing's
        times[16])."""
        t = np.zeros(17, np.float32)
        lib().sgpu_last_timing(self._ctx, t.ctypes.data, 17)
        return float(t[16])

    def match_guided(self, d1: np.ndarray, d2: np.ndarray, loc1: np.ndarray, loc2: np.ndarray,
                     H=None, F=None, distmax=0.7, ratiomax=0.8, hdistmax=32.0, fdistmax=16.0,
                     mbm=1, max_match=None, device_ptrs=None):
        """SiftMatchGPU::GetGuidedSiftMatch (SiftMatch.cpp:663-677): loc1/loc2 [n][2] (x, y),
        H/F 3x3 or None (defaults of SiftGPU.h:318-321).  device_ptrs = (d1, n1, d2, n2, loc1,
        loc2): int device pointers in place of the four arrays (SGPU_INPUT_DEVICE)."""
        if device_ptrs is not None:
            p1, n1, p2, n2, q1, q2 = device_ptrs
            flags = SGPU_INPUT_DEVICE
        else:
            d1 = np.ascontiguousarray(d1, np.uint8)
            d2 = np.ascontiguousarray(d2, np.uint8)
            l1 = np.ascontiguousarray(loc1, np.float32)
            l2 = np.ascontiguousarray(loc2, np.float32)
            n1, n2 = d1.shape[0], d2.shape[0]
            if l1.shape != (n1, 2) or l2.shape != (n2, 2):
                raise ValueError("locations must be [n][2] per descriptor set")
            p1, p2, q1, q2 = d1.ctypes.data, d2.ctypes.data, l1.ctypes.data, l2.ctypes.data
            flags = SGPU_INPUT_HOST
        hm = None if H is None else np.ascontiguousarray(H, np.float32).reshape(9)
        fm = None if F is None else np.ascontiguousarray(F, np.float32).reshape(9)
        max_match = n1 if max_match is None else max_match
        out = np.zeros((max(max_match, 1), 2), np.int32)
        m = lib().sgpu_match_guided(
            self._ctx, ctypes.c_void_p(p1), n1, ctypes.c_void_p(p2), n2, ctypes.c_void_p(q1),
            ctypes.c_void_p(q2),
            None if hm is None else hm.ctypes.data, None if fm is None else fm.ctypes.data,
            distmax, ratiomax, hdistmax, fdistmax, mbm, max_match, out.ctypes.data, flags)
        if m < 0:
            self._check(m, "sgpu_match_guided")
        return out[:m]

    # ---- multi-GPU (RCCL inside libsiftgpu)
    def comm_init(self, nranks: int, rank: int, uid: bytes):
        buf = (ctypes.c_uint8 * len(uid)).from_buffer_copy(uid)
        self._check(lib().sgpu_comm_init(self._ctx, nranks, rank, buf, len(uid)), "sgpu_comm_init")

    def allgather_i32(self, send: np.ndarray, nranks: int) -> np.ndarray:
        a = np.ascontiguousarray(send, np.int32)
        out = np.zeros(a.size * nranks, np.int32)
        self._check(lib().sgpu_comm_allgather_i32(self._ctx, a.ctypes.data, a.size, out.ctypes.data),
                    "sgpu_comm_allgather_i32")
        return out

    def allreduce_f64(self, v, op_max: bool) -> np.ndarray:
        a = np.ascontiguousarray(np.atleast_1d(v), np.float64).copy()
        self._check(lib().sgpu_comm_allreduce_f64(self._ctx, a.ctypes.data, a.size, 1 if op_max else 0),
                    "sgpu_comm_allreduce_f64")
        return a

    # ---- test hooks
    DEBUG_PARTS2, DEBUG_PARTS4, DEBUG_TINY_CAP, DEBUG_FUSED_MATCH = 1, 2, 4, 8
    DEBUG_EXACT_DESCRIPTOR = 16
    DEBUG_GAUSS_BLOCK = 32    # workgroup strip Gaussian (k_gauss_pk2)
    DEBUG_BAND_SHIFT = 20     # (rows << 20), rows < 2048: the wave kernels' forced band height (0: automatic)
    DEBUG_KEYED_MATCH = 64    # keyed matcher epilogue even when ratiomax <= 1
    DEBUG_FULL_COLUMNS = 128  # mutual matching decides every column, not only the matched ones
    DEBUG_DESC_DUAL = 256     # descriptors through the round-4 dual-cell kernel
    DEBUG_ORIENT_WAVE = 512   # orientation one wave per candidate for any candidate count
    DEBUG_GAUSS_TILE_ALWAYS = 1024  # every level (k_gauss_tile) and the extrema (k_extrema_tile) in tiles
    DEBUG_MATCH_REGSTAGE = 2048  # keyless matcher with register staging (k_match_rows<RAW>)
    DEBUG_PYR_SERIAL = 4096    # all pyramid octaves on one stream
    DEBUG_GAUSS_LONG_BANDS = 8192  # Gaussian bands of >= 4 chunks on every level
    DEBUG_DUO_ALWAYS = 16384   # paired-level Gaussian launches whatever the level size
    DEBUG_DUO_OFF = 32768      # no paired-level launches (one level per launch)
    DEBUG_GAUSS_TILE_OFF = 65536       # no tile launches (the wave-streaming level kernels)
    DEBUG_DESC_WIDE_OFF = 131072       # descriptors one wave per feature for every count
    DEBUG_DESC_WIDE_ALWAYS = 262144    # descriptors one workgroup per feature for every count
    DEBUG_EXTREMA_TILE_OFF = 524288    # extremum detection always through k_extrema_wave2

    def set_debug_flags(self, flags: int):
        """Per-context debug flags (sgpu_debug_set_flags; 0 = shipped configuration)."""
        self._check(lib().sgpu_debug_set_flags(self._ctx, flags), "sgpu_debug_set_flags")

    TRIO_OFF, TRIO_ON, TRIO_ALWAYS = 0, 1, 2
    PAIRS_FRONT, PAIRS_END = 0, 1

    def set_schedule(self, trio: int = 0, pairs: int = 1):
        """The batch pyramid's launch plan (sgpu_debug_set_schedule): three-level launches
        (TRIO_OFF, shipped; TRIO_ON: the size rule; TRIO_ALWAYS: wherever the widths and the
        decimation allow) and the octave's level pairs from its end (PAIRS_END, shipped) or its
        front (PAIRS_FRONT)."""
        self._check(lib().sgpu_debug_set_schedule(self._ctx, trio, pairs), "sgpu_debug_set_schedule")

    STRIPS_RULE, STRIPS_WAVE, STRIPS_COOP = 0, 1, 2

    def set_duo_strips(self, mode: int = 0):
        """Strip geometry of the paired-level launches (sgpu_debug_set_duo_strips): STRIPS_RULE
        (shipped: a workgroup's four waves share a 480-column strip where that issues fewer
        lane-columns and measured faster), STRIPS_WAVE (a 96-column strip per wave everywhere),
        STRIPS_COOP (the shared strip wherever it is compiled, at any width): the same levels."""
        self._check(lib().sgpu_debug_set_duo_strips(self._ctx, mode), "sgpu_debug_set_duo_strips")

    TOP_LEVEL_RULE, TOP_LEVEL_DENSE, TOP_LEVEL_LAZY = 0, 1, 2

    def set_top_level(self, mode: int = 0):
        """Every octave's last Gaussian level (sgpu_debug_set_top_level): TOP_LEVEL_DENSE (filtered
        for every pixel), TOP_LEVEL_LAZY (evaluated only around the top DoG level's candidates,
        wherever the wave-streaming extremum kernel runs) or TOP_LEVEL_RULE (shipped: lazy for
        batches too large for the tile extremum kernel): the same features."""
        self._check(lib().sgpu_debug_set_top_level(self._ctx, mode), "sgpu_debug_set_top_level")

    def top_level_at(self, image, octave, x, y):
        """The last Gaussian level's 3 x 3 values around (x, y) of (image, octave) by the sparse
        evaluation (sgpu_debug_top_level_at): a (3, 3) float32 array, [row, column]."""
        out = np.zeros(9, np.float32)
        self._check(lib().sgpu_debug_top_level_at(self._ctx, image, octave, x, y, out.ctypes.data),
                    "sgpu_debug_top_level_at")
        return out.reshape(3, 3)

    FEATURES_QUEUE, FEATURES_STATIC_ORIENTATION, FEATURES_STATIC_DESCRIPTOR, FEATURES_STATIC = 0, 1, 2, 3

    def set_feature_queue(self, mode: int = 0):
        """How a batch's orientation and descriptor kernels get their work
        (sgpu_debug_set_feature_queue): FEATURES_QUEUE (shipped: resident workgroups fed from work
        counters), FEATURES_STATIC (grids that cover the work) or one kernel of the two; same bits."""
        self._check(lib().sgpu_debug_set_feature_queue(self._ctx, mode), "sgpu_debug_set_feature_queue")

    def set_match_prune(self, on: bool = True):
        """Plain mutual matching's column side over the rows of set 1 that can change a listed
        column's decision (sgpu_debug_set_match_prune; on = shipped): the same pairs."""
        self._check(lib().sgpu_debug_set_match_prune(self._ctx, int(bool(on))),
                    "sgpu_debug_set_match_prune")

    def match_plan_stats(self):
        """The last match_batch / match_images call's plan (sgpu_debug_match_plan_stats): dict of
        items, sides, max_tiles (most 128-column tiles of an item) and max_chunks (most column
        chunks of a side)."""
        out = np.zeros(4, np.int64)
        self._check(lib().sgpu_debug_match_plan_stats(self._ctx, out.ctypes.data),
                    "sgpu_debug_match_plan_stats")
        return dict(zip(["items", "sides", "max_tiles", "max_chunks"], out.tolist()))

    @contextlib.contextmanager
    def exact_descriptors(self):
        """Within the block the descriptors come from the bit-exact kernel (the reference's fma
        order, the oracle's transcendentals) instead of the shipped relaxed-order one."""
        self.set_debug_flags(self.DEBUG_EXACT_DESCRIPTOR)
        try:
            yield self
        finally:
            self.set_debug_flags(0)

    def geometry(self):
        n = ctypes.c_int(0)
        dims = np.zeros(48, np.int32)
        lib().sgpu_debug_geometry(self._ctx, ctypes.byref(n), dims.ctypes.data, 16)
        return [tuple(dims[3 * i:3 * i + 3]) for i in range(n.value)]

    def gaussian(self, image, octave, level):
        w, h, wa = self.geometry()[octave]
        out = np.zeros(wa * h, np.float32)
        self._check(lib().sgpu_debug_gaussian(self._ctx, image, octave, level, out.ctypes.data),
                    "sgpu_debug_gaussian")
        return out

    def candidates(self):
        n = ctypes.c_int(0)
        lib().sgpu_debug_candidates(self._ctx, None, None, 0, ctypes.byref(n))
        ints = np.zeros((max(n.value, 1), 4), np.int32)
        fl = np.zeros((max(n.value, 1), 4), np.float32)
        self._check(lib().sgpu_debug_candidates(self._ctx, ints.ctypes.data, fl.ctypes.data,
                                                n.value, ctypes.byref(n)), "sgpu_debug_candidates")
        return ints[:n.value], fl[:n.value]
