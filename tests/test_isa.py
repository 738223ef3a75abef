"""Static checks on the built gfx950 code objects (CPU only: the objects are cross-compiled here).

* The descriptor histograms are LDS-only: k_descriptor_flat / k_descriptor_wide add their 64-bit
  fixed-point contributions with ds_add_u64 and contain no flat atomics (a
  round-5 variant of this kernel family faulted with an aperture violation, which a flat access
  through a generic pointer with an offset outside the LDS allocation produces, and an LDS
  instruction cannot: DESIGN.md 4.6).
* The shipped single-image kernels (tiles, the wide descriptor) use no scratch memory.
"""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "modify-sift-gpu_amd", "build")
LLVM = "/opt/rocm/lib/llvm/bin"


def _code_object(obj, td):
    fat = os.path.join(td, os.path.basename(obj) + ".fat")
    co = os.path.join(td, os.path.basename(obj) + ".co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fat}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}",
                           "--unbundle"])
    return co


def _functions(co):
    """{symbol: [instruction lines]} from llvm-objdump -d."""
    out = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], capture_output=True, text=True,
                         check=True).stdout
    funcs, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        elif cur and line.startswith("\t"):
            funcs[cur].append(line.strip())
    return funcs


def _kernel_meta(co):
    """{kernel name: private_segment_fixed_size} from the code object's metadata note."""
    out = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True,
                         check=True).stdout
    meta, name = {}, None
    for line in out.splitlines():
        m = re.search(r"\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", line)
        if m and name:
            meta[name] = int(m.group(1))
    return meta


def _need(path):
    if not os.path.exists(path) or not os.path.exists(f"{LLVM}/clang-offload-bundler"):
        pytest.skip(f"{path} not built (run __graft_entry__.build())")


def test_descriptor_histograms_are_lds_only():
    obj = os.path.join(BUILD, "sift_kernels.hip.o")
    _need(obj)
    with tempfile.TemporaryDirectory() as td:
        funcs = _functions(_code_object(obj, td))
    names = [n for n in funcs if "k_descriptor_flat" in n or "k_descriptor_wide" in n]
    assert len(names) >= 3, names   # k_descriptor_flat, k_descriptor_wide<4>, <8>
    for n in names:
        body = funcs[n]
        assert sum("ds_add_u64" in i for i in body) >= 8, n
        assert not [i for i in body if i.startswith("flat_atomic")], n


def test_single_image_kernels_use_no_scratch():
    with tempfile.TemporaryDirectory() as td:
        meta = {}
        for src in ("sift_kernels.hip.o", "sift_detect.hip.o", "sift_gauss_tile.hip.o"):
            obj = os.path.join(BUILD, src)
            _need(obj)
            meta.update(_kernel_meta(_code_object(obj, td)))
    picked = {k: v for k, v in meta.items()
              if any(s in k for s in ("k_gauss_tile", "k_descriptor_wide", "k_extrema_tile",
                                      "k_scan_single"))}
    assert len(picked) >= 10, sorted(meta)[:20]
    assert all(v == 0 for v in picked.values()), {k: v for k, v in picked.items() if v}
