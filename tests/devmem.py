"""Device buffers for the tests of the library's device-pointer entry points (SGPU_INPUT_DEVICE):
hipMalloc / hipMemcpy / hipFree through ctypes, on the HIP runtime that libsiftgpu.so has already
mapped into the process.  Its path is read from the process's mappings after sgpu.lib(), so
dlopen returns the mapped copy's handle and no second runtime is loaded: with a second copy of
libamdhip64 in the process (what importing torch brings) a context has found no device
(bench.py), and memory of one copy means nothing to the other.  A plain helper, not a conftest."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

import sgpu

H2D, D2H = 1, 2   # hipMemcpyHostToDevice, hipMemcpyDeviceToHost
ALLOC_ROUND = 256

_HIP = None


def mapped_hip_path():
    """The file of the libamdhip64 this process has mapped (exactly one, or an error)."""
    sgpu.lib()
    paths = set()
    with open("/proc/self/maps") as f:
        for line in f:
            part = line.split(None, 5)
            if len(part) == 6 and "libamdhip64.so" in part[5]:
                paths.add(part[5].strip())
    if len(paths) != 1:
        raise RuntimeError(f"expected one mapped libamdhip64, found {sorted(paths)}")
    return paths.pop()


def hip():
    global _HIP
    if _HIP is None:
        L = ctypes.CDLL(mapped_hip_path())
        vp = ctypes.c_void_p
        L.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
        L.hipFree.argtypes = [vp]
        L.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
        L.hipSetDevice.argtypes = [ctypes.c_int]
        _HIP = L
    return _HIP


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with hipError {rc}")


class DeviceBuffer:
    """One hipMalloc allocation of `size` bytes (rounded up to ALLOC_ROUND) on `device`."""

    def __init__(self, size: int, device: int = 0):
        self.size = (max(int(size), 1) + ALLOC_ROUND - 1) // ALLOC_ROUND * ALLOC_ROUND
        _ok(hip().hipSetDevice(device), "hipSetDevice")
        p = ctypes.c_void_p()
        _ok(hip().hipMalloc(ctypes.byref(p), self.size), "hipMalloc")
        self.base = int(p.value)

    def _span(self, offset, nbytes):
        if offset < 0 or nbytes < 0 or offset + nbytes > self.size or not self.base:
            raise ValueError(f"[{offset}, {offset + nbytes}) leaves the {self.size}-byte allocation")
        return self.base + offset

    def upload(self, host: np.ndarray, offset: int = 0) -> int:
        """Copy the array's bytes to base + offset; returns that device address."""
        a = np.ascontiguousarray(host)
        dst = self._span(offset, a.nbytes)
        _ok(hip().hipMemcpy(dst, a.ctypes.data, a.nbytes, H2D), "hipMemcpy (to the device)")
        return dst

    def download(self, shape, dtype, offset: int = 0) -> np.ndarray:
        out = np.empty(shape, dtype)
        src = self._span(offset, out.nbytes)
        _ok(hip().hipMemcpy(out.ctypes.data, src, out.nbytes, D2H), "hipMemcpy (to the host)")
        return out

    def free(self):
        if self.base:
            _ok(hip().hipFree(self.base), "hipFree")
            self.base = 0


@contextlib.contextmanager
def uploaded(host: np.ndarray, offset: int = 0, device: int = 0):
    """The array's bytes in device memory, `offset` bytes into an allocation of offset + nbytes
    (rounded up): yields the device address of the first byte; the allocation is freed on exit.
    Every byte of [address, address + nbytes) lies inside the allocation."""
    buf = DeviceBuffer(offset + np.ascontiguousarray(host).nbytes, device)
    try:
        yield buf.upload(host, offset)
    finally:
        buf.free()


@contextlib.contextmanager
def allocated(nbytes: int, device: int = 0):
    """An uninitialised device allocation: yields the DeviceBuffer; freed on exit."""
    buf = DeviceBuffer(nbytes, device)
    try:
        yield buf
    finally:
        buf.free()
