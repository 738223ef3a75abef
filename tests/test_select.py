"""Preemptive matching on the CPU: the selection rule of csrc/sift_select.h, the C declarations and
what the library and the binding refuse without a device.

tests/abi/select_check.cpp includes only sift_select.h and is built with g++ as a stand-alone
program under AddressSanitizer and UBSan.  In file mode it runs sgsel::select_host on the cases of
tests/select_cases.py -- the ones the GPU test gives k_select_top_scale -- and the selections are
compared with NumPy: np.sort(np.argsort(-key, kind="stable")[:top]), key being the order key
computed in NumPy on the uint32 view of the scales."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import select_cases as SC
import sgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modify-sift-gpu_amd", "csrc")


@pytest.fixture(scope="module")
def select_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("select_check") / "select_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "abi", "select_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_select_host_self_test_under_sanitizers(select_check):
    r = subprocess.run([select_check], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "select ok" in r.stdout, r.stdout + r.stderr


def _run(select_check, tmp_path, cases):
    """cases: [(scales flat, stride, n, top)] -> the selections select_host wrote."""
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for flat, stride, n, top in cases:
            buf = np.zeros(n * stride, np.float32)
            buf[:len(flat)] = flat[:n * stride]
            f.write(np.array([n, stride, top], np.int32).tobytes())
            f.write(buf.tobytes())
    r = subprocess.run([select_check, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(dst, np.int32)
    out, at = [], 0
    for _ in cases:
        m = int(raw[at])
        out.append(raw[at + 1:at + 1 + m])
        at += 1 + m
    assert at == len(raw)
    return out


def test_select_host_equals_numpy_on_the_shared_cases(select_check, tmp_path):
    labels, cases, want = [], [], []
    for top in SC.TOPS:
        for label, scale in SC.sets_for(top):
            for stride in (1, 4):
                if stride == 4 and not label.startswith(("random", "three", "caller")):
                    continue
                labels.append((label, top, stride))
                cases.append((SC.strided(scale, stride, 0) if stride > 1 else scale, stride,
                              len(scale), top))
                want.append(SC.numpy_select(scale, top))
    got = _run(select_check, tmp_path, cases)
    for lab, g, w in zip(labels, got, want):
        assert np.array_equal(g, w), (lab, g[:10], w[:10])
    # the cases do what they are there for: a tie group that straddles the cut, taken in part
    scale = SC.pattern("three", 257, 100, 1)
    key = SC.order_key(scale)
    sel = SC.numpy_select(scale, 100)
    T = np.sort(key)[::-1][99]
    taken, group = int((key[sel] == T).sum()), int((key == T).sum())
    assert 0 < taken < group and not np.array_equal(sel, np.arange(257 - 100, 257))
    # caller data: the order is order_key's -- +inf first, then the positive NaN above it...
    cd = SC.caller_data()
    first = SC.numpy_select(cd, 1)[0]
    assert np.isnan(cd[first]) and not np.signbit(cd[first])
    last = np.argsort(SC.order_key(cd).astype(np.int64), kind="stable")[0]
    assert np.isnan(cd[last]) and np.signbit(cd[last])
    k = SC.order_key(np.array([-0.0, 0.0], np.float32))
    assert k[0] < k[1]


def test_select_header_includes_no_hip():
    src = open(os.path.join(CSRC, "sift_select.h")).read()
    assert "hip" not in "".join(l for l in src.splitlines(True) if l.lstrip().startswith("#include"))


def test_header_is_plain_c_and_declares_prematch(tmp_path):
    src = os.path.join(ROOT, "tests", "abi", "prematch_abi.c")
    obj = str(tmp_path / "prematch_abi.o")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I",
                        os.path.join(ROOT, "include"), "-c", "-o", obj, src],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    syms = subprocess.check_output(["nm", obj], text=True)
    for name in ("sgpu_select_top_scale_batch", "sgpu_select_top_scale_images",
                 "sgpu_prematch_batch", "sgpu_prematch_images"):
        assert f" U {name}" in syms, name


def test_null_context_needs_no_device():
    L = sgpu.lib()
    off = (ctypes.c_int64 * 2)(0, 0)
    sub = (ctypes.c_int64 * 2)(7, 7)
    idx = (ctypes.c_int * 1)(7)
    counts = (ctypes.c_int * 1)(7)
    assert L.sgpu_select_top_scale_batch(None, None, 1, off, 1, 100, idx, sub, 0) == sgpu.SGPU_EINVAL
    assert L.sgpu_select_top_scale_images(None, 100, idx, sub) == sgpu.SGPU_EINVAL
    assert L.sgpu_prematch_batch(None, None, None, 1, off, 1, None, 0, 100, 0.7, 0.8, 1, counts,
                                 None, 0, 0) == sgpu.SGPU_EINVAL
    assert L.sgpu_prematch_images(None, None, 0, 100, 0.7, 0.8, 1, counts, None, 0) == sgpu.SGPU_EINVAL
    assert list(sub) == [7, 7] and idx[0] == 7 and counts[0] == 7


def test_binding_rejects_wrong_shapes():
    """The binding's ValueErrors come before any C call: no device needed."""
    ctx = sgpu.SiftContext.__new__(sgpu.SiftContext)
    ctx._ctx = None
    ctx.batch = 0
    q = np.zeros((10, 128), np.uint8)
    sc = np.ones(10, np.float32)
    with pytest.raises(ValueError):
        ctx.select_top_scale(sc, [0, 4, 11], 3)               # more rows than scales
    with pytest.raises(ValueError):
        ctx.select_top_scale(sc, [0, 4, 10], 3, stride=2)     # ... at this stride
    with pytest.raises(ValueError):
        ctx.select_top_scale(sc, [0, 4, 10], 3, stride=0)
    with pytest.raises(ValueError):
        ctx.select_top_scale(sc, [], 3)
    with pytest.raises(ValueError):
        ctx.prematch_batch(q, sc, [0, 4, 11])                 # offsets past the descriptors
    with pytest.raises(ValueError):
        ctx.prematch_batch(q, sc[:9], [0, 4, 10])             # ... past the scales
    with pytest.raises(ValueError):
        ctx.prematch_batch(q.reshape(-1)[:-1], sc, [0, 4, 10])   # not rows of 128 bytes
    with pytest.raises(ValueError):
        ctx.prematch_batch(q, sc, [0, 4, 10], pairs=[(0, 1, 1)])  # not [npairs][2]
