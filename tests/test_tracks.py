"""Feature tracks on the CPU: the rule of csrc/sift_tracks.h, the C declarations and what the library
and the binding refuse without a device.

tests/abi/tracks_check.cpp includes only sift_tracks.h and is built with g++ as a stand-alone
program under AddressSanitizer and UBSan.  In file mode it runs sgtrk::tracks_host on the cases of
tests/track_cases.py -- the ones the GPU test gives sgpu_tracks_batch -- and the results are
compared with the NumPy expectation, which propagates minimum labels and knows no union-find."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sgpu
import track_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modify-sift-gpu_amd", "csrc")


@pytest.fixture(scope="module")
def tracks_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tracks_check") / "tracks_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tests", "abi", "tracks_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_cases_do_what_they_are_there_for():
    TC.check_cases_do_their_job()


def test_tracks_host_self_test_under_sanitizers(tracks_check):
    r = subprocess.run([tracks_check], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "tracks ok" in r.stdout, r.stdout + r.stderr


def same(got, want, what):
    assert got.T == want.T, what
    for name in ("track", "offsets", "rows", "stats"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), (what, name)


def test_tracks_host_equals_numpy_on_the_shared_cases(tracks_check, tmp_path):
    runs = [(name, ml) for name in TC.NAMES for ml in TC.MIN_LENGTHS]
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    TC.write_cases(src, [(TC.cases()[name], ml) for name, ml in runs])
    r = subprocess.run([tracks_check, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for run, got in zip(runs, TC.read_results(dst, len(runs))):
        same(got, TC.expected(*run), run)


def test_tracks_header_includes_no_hip():
    src = open(os.path.join(CSRC, "sift_tracks.h")).read()
    assert "hip" not in "".join(l for l in src.splitlines(True) if l.lstrip().startswith("#include"))
    assert "namespace sgtrk" in src and "SGTRK_HD" in src


def test_header_is_plain_c_and_declares_tracks(tmp_path):
    src = os.path.join(ROOT, "tests", "abi", "tracks_abi.c")
    obj = str(tmp_path / "tracks_abi.o")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-Werror", "-I",
                        os.path.join(ROOT, "include"), "-c", "-o", obj, src],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    syms = subprocess.check_output(["nm", obj], text=True)
    for name in ("sgpu_tracks_batch", "sgpu_tracks_images"):
        assert f" U {name}" in syms, name


def test_null_context_needs_no_device():
    L = sgpu.lib()
    off = (ctypes.c_int64 * 3)(0, 2, 4)
    pairs = (ctypes.c_int * 2)(0, 1)
    matches = (ctypes.c_int * 2)(1, 1)
    counts = (ctypes.c_int * 1)(1)
    track = (ctypes.c_int * 4)(7, 7, 7, 7)
    offs = (ctypes.c_int64 * 3)(7, 7, 7)
    rows = (ctypes.c_int * 4)(7, 7, 7, 7)
    stats = (ctypes.c_longlong * 4)(7, 7, 7, 7)
    assert L.sgpu_tracks_batch(None, off, 2, pairs, 1, matches, counts, 2, track, offs, rows,
                               stats) == sgpu.SGPU_EINVAL
    assert L.sgpu_tracks_images(None, pairs, 1, matches, counts, 2, track, offs, rows,
                                stats) == sgpu.SGPU_EINVAL
    assert list(track) + list(offs) + list(rows) + list(stats) == [7] * 15


def test_binding_rejects_wrong_shapes():
    """The binding's ValueErrors come before any C call: no device needed."""
    ctx = sgpu.SiftContext.__new__(sgpu.SiftContext)
    ctx._ctx = None
    ctx.batch = 0
    m = np.zeros((1, 2), np.int32)
    with pytest.raises(ValueError):
        ctx.tracks_batch([], [(0, 1)], [m])                      # no offsets at all
    with pytest.raises(ValueError):
        ctx.tracks_batch([0, 4, 3], [(0, 1)], [m])               # decreasing offsets
    with pytest.raises(ValueError):
        ctx.tracks_batch([0, 4, 8], [(0, 1, 1)], [m])            # not [npairs][2]
    with pytest.raises(ValueError):
        ctx.tracks_batch([0, 4, 8], [(0, 1)], [m, m])            # a match list too many
    with pytest.raises(ValueError):
        ctx.tracks_batch([0, 4, 8], [(0, 1)], [np.zeros((2, 3), np.int32)])   # not [m][2]
    with pytest.raises(ValueError):
        ctx.tracks_batch([0, 4, 8], [(0, 1)], [m], min_length=1)
    with pytest.raises(ValueError):
        ctx.tracks_images([(0, 1)], [])
    with pytest.raises(ValueError):
        sgpu.track_features([8], [0, 4, 8])                      # a row past the sets
    s, f = sgpu.track_features([0, 3, 4, 7], [0, 4, 4, 8])
    assert s.tolist() == [0, 0, 2, 2] and f.tolist() == [0, 3, 0, 3]
    assert sgpu.Tracks._fields == ("track_of_row", "offsets", "rows", "stats")
    assert (sgpu.SGPU_TRACK_NONE, sgpu.SGPU_TRACK_INCONSISTENT) == (-1, -2)
