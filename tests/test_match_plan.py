"""Host planner of the grouped pair matcher (csrc/sift_match_plan.h), checked without a GPU: the
stand-alone program tests/abi/match_plan_check.cpp includes only that header, is built with
AddressSanitizer and UBSan and asserts that the work items cover every (pair, direction, panel,
chunk) exactly once, that the chunks tile the columns, that empty sets yield no items, that no
part / decision offset overlaps another or exceeds the reported sizes, and that one pair of large
sets still yields at least as many items as the chip has compute units."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_match_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "match_plan_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "modify-sift-gpu_amd", "csrc"),
                        os.path.join(ROOT, "tests", "abi", "match_plan_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match plan ok" in r.stdout


def test_plan_header_includes_no_hip():
    src = open(os.path.join(ROOT, "modify-sift-gpu_amd", "csrc", "sift_match_plan.h")).read()
    assert "hip" not in "".join(l for l in src.splitlines(True) if l.lstrip().startswith("#include"))
