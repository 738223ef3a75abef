"""Launch planner of the Gaussian pyramid (csrc/sift_pyramid_plan.h), checked without a GPU: the
stand-alone program tests/abi/pyramid_plan_check.cpp includes only that header and sift_params.h
(the real filter widths and octave geometry), is built with AddressSanitizer and UBSan, and asserts
(a) over the suite's shapes and the benchmark's, -d 3 and 4 and every combination of the rule
switches, that each level is in exactly one launch, that a level's input is written by an earlier
launch or an earlier level of the same multi-level launch, that multi-level launches appear only
where a kernel is compiled for them and never with pairing off, and the side-stream layout's event
marks; (b) the exact launch lists of the three benchmark shapes under the shipped rules."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modify-sift-gpu_amd", "csrc")


def test_pyramid_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "pyramid_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-Wall", "-I", CSRC,
                        os.path.join(ROOT, "tests", "abi", "pyramid_plan_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pyramid plan ok" in r.stdout


def test_plan_header_includes_no_hip():
    src = open(os.path.join(CSRC, "sift_pyramid_plan.h")).read()
    assert "hip" not in "".join(l for l in src.splitlines(True) if l.lstrip().startswith("#include"))

