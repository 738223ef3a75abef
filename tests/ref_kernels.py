"""ctypes binding of oracle/_ref/libref_kernels*.so: the reference's own CUDA kernels, run on
the CPU by oracle/cuda_host (oracle/ref_driver.cpp) -- test infrastructure only.

The libraries exist only where oracle/Makefile found a checkout of the reference; available()
says whether they do.  Every function runs one ProgramCU:: stage on the arrays passed in.  The
two builds differ in -ffp-contract (off / fast); `fast=True` selects the second."""
from __future__ import annotations

import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = {False: os.path.join(ROOT, "oracle", "_ref", "libref_kernels.so"),
         True: os.path.join(ROOT, "oracle", "_ref", "libref_kernels_fast.so")}
SKIP_REASON = "reference kernels not built (oracle/_ref: no reference checkout at build time)"
_LIBS = {}


def available():
    return all(os.path.exists(p) for p in PATHS.values())


def lib(fast=False):
    if fast not in _LIBS:
        L = ctypes.CDLL(PATHS[fast])
        vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.ref_settings.argtypes = [i, i, i, i, f, f, f, f, i, i]
        L.ref_stats.argtypes = [vp]
        L.ref_filter_kernel.argtypes = [f, vp]
        L.ref_filter.argtypes = [vp, i, i, f, vp]
        L.ref_sample_d.argtypes = [vp, i, i, i, vp, i, i]
        L.ref_sample_u.argtypes = [vp, i, i, i, vp]
        L.ref_reduce_channel.argtypes = [vp, i, i, i, vp]
        L.ref_byte_to_float.argtypes = [vp, i, i, vp]
        L.ref_dog.argtypes = [vp, vp, i, i, vp, vp]
        L.ref_key.argtypes = [vp, vp, vp, i, i, f, f, vp]
        L.ref_init_hist.argtypes = [vp, i, i, i, vp]
        L.ref_reduce_hist.argtypes = [vp, i, i, i, vp]
        L.ref_gen_list.argtypes = [vp, i, vp, i, i]
        L.ref_orientation.argtypes = [vp, i, vp, vp, i, i, f, f, i]
        L.ref_descriptor.argtypes = [vp, i, vp, i, i, i, vp]
        L.ref_match_stages.argtypes = [vp, i, vp, i, vp, vp, vp, vp, f, f, f, f, i, vp, vp, vp]
        _LIBS[fast] = L
    return _LIBS[fast]


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def settings(fast=False, subpixel=1, max_orientation=2, fixed_orientation=0, keep_sign=0,
             filter_width_factor=4.0, orientation_gaussian_factor=1.5,
             orientation_window_factor=2.0, descriptor_window_factor=3.0, normalized=1,
             dynamic_indexing=0):
    """The GlobalUtil settings the stage functions read (defaults: the reference's)."""
    lib(fast).ref_settings(subpixel, max_orientation, fixed_orientation, keep_sign,
                           filter_width_factor, orientation_gaussian_factor,
                           orientation_window_factor, descriptor_window_factor, normalized,
                           dynamic_indexing)


def stats(fast=False, reset=True):
    """{launches, blocks, oob (out-of-range 1D fetches), clamped (2D)} since the last reset."""
    out = (ctypes.c_long * 4)()
    lib(fast).ref_stats(out)
    if reset:
        lib(fast).ref_reset_stats()
    return dict(zip(("launches", "blocks", "oob", "clamped"), out))


def filter_kernel(sigma, fast=False):
    k = np.zeros(33, np.float32)
    n = lib(fast).ref_filter_kernel(sigma, k.ctypes.data)
    return k[:n]


def filter_image(img, sigma, fast=False):
    src = _f32(img)
    h, w = src.shape
    dst = np.zeros_like(src)
    lib(fast).ref_filter(src.ctypes.data, w, h, sigma, dst.ctypes.data)
    return dst


def sample_d(img, log_scale, dw, dh, fast=False):
    src = _f32(img)
    h, w = src.shape
    dst = np.zeros((dh, dw), np.float32)
    lib(fast).ref_sample_d(src.ctypes.data, w, h, log_scale, dst.ctypes.data, dw, dh)
    return dst


def sample_u(img, log_scale, fast=False):
    src = _f32(img)
    h, w = src.shape
    dst = np.zeros((h << log_scale, w << log_scale), np.float32)
    lib(fast).ref_sample_u(src.ctypes.data, w, h, log_scale, dst.ctypes.data)
    return dst


def reduce_channel(rgba, convert_rgb, fast=False):
    src = _f32(rgba)
    h, w, c = src.shape
    assert c == 4
    dst = np.zeros((h, w), np.float32)
    lib(fast).ref_reduce_channel(src.ctypes.data, w, h, int(convert_rgb), dst.ctypes.data)
    return dst


def byte_to_float(img, fast=False):
    src = np.ascontiguousarray(img, np.uint8)
    h, w = src.shape
    dst = np.zeros((h, w), np.float32)
    lib(fast).ref_byte_to_float(src.ctypes.data, w, h, dst.ctypes.data)
    return dst


def dog(prev, cur, gradient=False, fast=False):
    """(dog [h, w], gradient [h, w, 2] = (magnitude, angle) of `cur`, or None)."""
    p, c = _f32(prev), _f32(cur)
    h, w = c.shape
    d = np.zeros((h, w), np.float32)
    g = np.zeros((h, w, 2), np.float32) if gradient else None
    lib(fast).ref_dog(p.ctypes.data, c.ctypes.data, w, h, d.ctypes.data,
                      g.ctypes.data if gradient else None)
    return d, g


def key(dp, dc, dn, tdog, tedge, fast=False):
    """ComputeKEY's key image [h, w, 4] = (+-1 or 0, dx, dy, ds)."""
    dp, dc, dn = _f32(dp), _f32(dc), _f32(dn)
    h, w = dc.shape
    k = np.zeros((h, w, 4), np.float32)
    lib(fast).ref_key(dp.ctypes.data, dc.ctypes.data, dn.ctypes.data, w, h, tdog, tedge,
                      k.ctypes.data)
    return k


def feature_list(key_img, widths, fast=False):
    """InitHistogram / ReduceHistogram down `widths` (oracle_hist_widths: finest first, the last
    is the row-reduction level) and GenerateList back up: the per-level list [n, 4] int32
    (col, row, 0, 0).  The seeding between the two (one entry per count of the coarsest level)
    is host code of PyramidCU::GenerateFeatureList, restated here."""
    k = _f32(key_img)
    h, ws, _ = k.shape
    L = lib(fast)
    hists = [np.zeros((h, widths[0], 4), np.int32)]
    L.ref_init_hist(k.ctypes.data, ws, h, widths[0], hists[0].ctypes.data)
    for wd in widths[1:]:
        nxt = np.zeros((h, wd, 4), np.int32)
        L.ref_reduce_hist(hists[-1].ctypes.data, hists[-1].shape[1], h, wd, nxt.ctypes.data)
        hists.append(nxt)
    top = hists[-1]
    assert top.shape[1] == 1
    flat = top.reshape(-1)
    entries = [(ii % 4, ii // 4, jj, 0) for ii in range(flat.size) for jj in range(int(flat[ii]))]
    lst = np.array(entries, np.int32).reshape(-1, 4)
    if len(lst):
        for hist in hists[-2::-1]:
            L.ref_gen_list(lst.ctypes.data, len(lst), hist.ctypes.data, hist.shape[1], h)
    return lst, hists


def orientation(lst, got, key_img, sigma, sigma_step, existing=False, fast=False):
    """ComputeOrientation on a per-level list (int32 [n, 4]) or, with existing, float keys
    [n, 4]; returns float32 [n, 4] (x, y, scale, packed orientations or angle)."""
    buf = np.ascontiguousarray(lst, np.float32 if existing else np.int32).copy()
    g = _f32(got)
    h, w, _ = g.shape
    kp = _f32(key_img) if key_img is not None else None
    if len(buf):
        lib(fast).ref_orientation(buf.ctypes.data, len(buf), g.ctypes.data,
                                  kp.ctypes.data if kp is not None else None, w, h, sigma,
                                  sigma_step, int(existing))
    return buf.view(np.float32)


def descriptor(keys, got, rect=False, fast=False):
    k = _f32(keys).reshape(-1, 4)
    g = _f32(got)
    h, w, _ = g.shape
    d = np.zeros((len(k), 128), np.float32)
    if len(k):
        lib(fast).ref_descriptor(k.ctypes.data, len(k), g.ctypes.data, w, h, int(rect),
                                 d.ctypes.data)
    return d


def match_stages(d1, d2, distmax=0.7, ratiomax=0.8, mbm=1, loc1=None, loc2=None, H=None, F=None,
                 hdistmax=32.0, fdistmax=16.0, fast=False, want_dot=True):
    """MultiplyDescriptor (MultiplyDescriptorG with locations) -> GetRowMatch -> GetColMatch:
    (row [n1], col [n2] or None, dot [n1, n2] or None)."""
    d1 = np.ascontiguousarray(d1, np.uint8)
    d2 = np.ascontiguousarray(d2, np.uint8)
    n1, n2 = len(d1), len(d2)
    row = np.zeros(n1, np.int32)
    col = np.zeros(n2, np.int32)
    dot = np.zeros((n1, n2), np.int32) if want_dot else None
    guided = loc1 is not None
    if guided:
        loc1, loc2, H, F = _f32(loc1), _f32(loc2), _f32(H), _f32(F)
    lib(fast).ref_match_stages(d1.ctypes.data, n1, d2.ctypes.data, n2,
                               loc1.ctypes.data if guided else None,
                               loc2.ctypes.data if guided else None,
                               H.ctypes.data if guided else None,
                               F.ctypes.data if guided else None, hdistmax, fdistmax, distmax,
                               ratiomax, int(mbm), row.ctypes.data, col.ctypes.data,
                               dot.ctypes.data if want_dot else None)
    return row, (col if mbm else None), dot


def pairs(row, col, max_match=None):
    """The list SiftMatchCU::GetBestMatch builds from the two kernels' results: ascending i,
    row[i] >= 0 and, with the mutual check, col[row[i]] == i; at most max_match."""
    out = [(i, int(j)) for i, j in enumerate(row) if j >= 0 and (col is None or col[j] == i)]
    out = out[:len(row) if max_match is None else max_match]
    return np.array(out, np.int32).reshape(-1, 2)


def match(d1, d2, distmax=0.7, ratiomax=0.8, mbm=1, max_match=None, **guided):
    """What SiftMatchCU::GetSiftMatch / GetGuidedSiftMatch return, with the NULL-matrix
    defaults of SiftMatchGPU::GetGuidedSiftMatch applied by the caller."""
    row, col, _ = match_stages(d1, d2, distmax, ratiomax, mbm, want_dot=False, **guided)
    return pairs(row, col, max_match)
