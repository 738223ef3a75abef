"""Strip plan of the paired Gaussian's cooperative form (csrc/sift_gauss_coop_plan.h), checked
without a GPU: the stand-alone program tests/abi/duo_coop_plan_check.cpp includes only that header,
is built with AddressSanitizer and UBSan, and asserts for every level width that is a multiple of 4
from 8 to 4,100 and every compiled filter pair that each output column has exactly one owner, that
every mid column stage B reads was written exactly once with the clamp-to-edge column, that nothing
leaves the workgroup's 512-column row and that strips start on multiples of 32 columns."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_duo_coop_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "duo_coop_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "modify-sift-gpu_amd", "csrc"),
                        os.path.join(ROOT, "tests", "abi", "duo_coop_plan_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "duo coop plan ok" in r.stdout


def test_plan_header_includes_no_hip():
    src = open(os.path.join(ROOT, "modify-sift-gpu_amd", "csrc", "sift_gauss_coop_plan.h")).read()
    assert "hip" not in "".join(l for l in src.splitlines(True) if l.lstrip().startswith("#include"))
