"""The verify chain's C interface (sgpu_verify_params, sgpu_default_verify_params,
sgpu_verify_batch, sgpu_verify_images), on the CPU: include/sgpu.h stays plain C with the new
declarations in it, and the parts of the library that need no device behave as the header says."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sgpu
from sgpu_types import SgpuVerifyParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the header's documented defaults, field by field
DEFAULTS = dict(distmax=0.7, ratiomax=0.8, mutual_best_match=1, max_match=4096, h_threshold=2.0,
                f_threshold=4.0, hdistmax=2.0, fdistmax=4.0, iterations=512, seed=0, refine_rounds=3)


def test_header_is_plain_c_and_declares_the_verify_chain(tmp_path):
    src = os.path.join(ROOT, "tests", "abi", "verify_abi.c")
    obj = str(tmp_path / "verify_abi.o")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I",
                        os.path.join(ROOT, "include"), "-c", "-o", obj, src],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    syms = subprocess.check_output(["nm", obj], text=True)
    for name in ("sgpu_default_verify_params", "sgpu_verify_batch", "sgpu_verify_images"):
        assert f" U {name}" in syms, name


def test_struct_mirror_matches_the_header_layout():
    assert [f[0] for f in SgpuVerifyParams._fields_] == list(DEFAULTS)
    assert ctypes.sizeof(SgpuVerifyParams) == 44 and SgpuVerifyParams.refine_rounds.offset == 40


def test_defaults_and_null_context_need_no_device():
    L = sgpu.lib()
    vp = SgpuVerifyParams()
    ctypes.memset(ctypes.byref(vp), 0xA5, ctypes.sizeof(vp))
    L.sgpu_default_verify_params(ctypes.byref(vp))
    for name, want in DEFAULTS.items():
        got = getattr(vp, name)
        assert got == (ctypes.c_float(want).value if isinstance(want, float) else want), name
    L.sgpu_default_verify_params(None)   # a NULL struct is ignored
    off = (ctypes.c_int64 * 2)(0, 0)
    counts = (ctypes.c_int * 1)()
    H = (ctypes.c_float * 9)()
    rc = L.sgpu_verify_batch(None, None, None, off, 1, None, 0, ctypes.byref(vp), H, None, None,
                             None, None, None, 0, counts, sgpu.SGPU_INPUT_HOST)
    assert rc == sgpu.SGPU_EINVAL
    rc = L.sgpu_verify_images(None, None, 0, ctypes.byref(vp), H, None, None, None, None, None, 0,
                              counts)
    assert rc == sgpu.SGPU_EINVAL
    # the binding fills the same defaults and rejects an unknown field before any device call
    p = sgpu.SiftContext.verify_params(seed=7, refine_rounds=0)
    assert (p.seed, p.refine_rounds, p.iterations, p.max_match) == (7, 0, 512, 4096)
    with pytest.raises(TypeError):
        sgpu.SiftContext.verify_params(rounds=3)


def test_binding_rejects_wrong_shapes():
    """The binding's ValueErrors come before any C call: no device needed."""
    ctx = sgpu.SiftContext.__new__(sgpu.SiftContext)
    ctx._ctx = None
    ctx.batch = 0
    q = np.zeros((10, 128), np.uint8)
    loc = np.zeros((10, 2), np.float32)
    with pytest.raises(ValueError):
        ctx.verify_batch(q, np.zeros((10, 4), np.float32), [0, 4, 10], [(0, 1)])
    with pytest.raises(ValueError):
        ctx.verify_batch(q, loc, [0, 4, 11], [(0, 1)])
    with pytest.raises(ValueError):
        ctx.verify_batch(q, loc, [0, 4, 10], [(0, 1)], H=False, F=False)
    with pytest.raises(ValueError):
        ctx.verify_images([(0, 1)], H=False, F=False)
