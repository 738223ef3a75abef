"""Time SiftContext.tracks_batch against the host loop of the same rule.

Workload: 64 sets of 8,000 rows, all 2,016 pairs; planted points as in the random case of
tests/track_cases.py: every set sees 8,000 of the points, a pair matches about 70 % of its common
points and adds 2 % wrong matches.  The same input goes two ways:

  (a) device: SiftContext.tracks_batch -- sgpu_last_timing's times[15] (device) and the wall time
      of the call, upload and downloads included;
  (b) host: sgtrk::tracks_host through the stand-alone program tests/abi/tracks_check.cpp, built
      here with g++ -O2, which times the loop alone (no file reading).

It checks that both give the same tracks and writes <out>/tracks_time_<tag>.json with median
[min, max] of the times, the upload size and the counts.

    python tests/tracks_time.py [--tag TAG] [--repeats 10] [--sets 64] [--rows 8000] [--out DIR]

A plain script, not a test.  The GPU work runs in a child process under a time limit."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "modify-sift-gpu_amd", "python"))


def stats(v):
    import numpy as np
    a = np.asarray(v, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
            "n": int(len(a))}


def workload(nsets, rows, seed=4203):
    """(Case, points): every set sees `rows` of the points, each point about 3.5 sets."""
    import numpy as np
    import track_cases as TC
    rng = np.random.Generator(np.random.PCG64(seed))
    npoints = int(nsets * rows / 3.5)
    row_of = np.full((nsets, npoints), -1, np.int32)
    for s in range(nsets):
        row_of[s, rng.choice(npoints, rows, replace=False)] = rng.permutation(rows).astype(np.int32)
    a, b = np.triu_indices(nsets, 1)
    order = rng.permutation(len(a))
    pairs = np.stack([a[order], b[order]], axis=1).astype(np.int32)
    matches = []
    for x, y in pairs:
        common = np.flatnonzero((row_of[x] >= 0) & (row_of[y] >= 0))
        keep = common[rng.random(len(common)) < 0.7]
        wrong = rng.integers(0, rows, (rng.binomial(len(common), 0.02), 2)).astype(np.int32)
        matches.append(np.concatenate([np.stack([row_of[x, keep], row_of[y, keep]], axis=1), wrong]))
    return TC.Case(np.arange(nsets + 1, dtype=np.int64) * rows, pairs, matches), npoints


def host_loop(case, min_length, repeats, tmp):
    """[ms] of tracks_host alone, and its results."""
    import track_cases as TC
    exe, src, dst = (os.path.join(tmp, n) for n in ("tracks_check", "cases.bin", "out.bin"))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "modify-sift-gpu_amd", "csrc"),
                           os.path.join(ROOT, "tests", "abi", "tracks_check.cpp"), "-o", exe])
    TC.write_cases(src, [(case, min_length)] * repeats)
    out = subprocess.check_output([exe, src, dst], text=True)
    ms = [float(m) for m in re.findall(r"tracks_host ([0-9.]+) ms", out)]
    assert len(ms) == repeats
    return ms, TC.read_results(dst, repeats)[0]


def child(args):
    import numpy as np
    import sgpu
    case, npoints = workload(args.sets, args.rows)
    total = sum(len(m) for m in case.matches)
    upload = (len(case.offsets) + len(case.pairs) + 1) * 8 + len(case.pairs) * 8 + total * 8
    ctx = sgpu.SiftContext(0)
    wall, dev = [], []
    got = None
    for i in range(2 + args.repeats):
        t0 = time.perf_counter()
        got = ctx.tracks_batch(case.offsets, case.pairs, case.matches, args.min_length)
        w = (time.perf_counter() - t0) * 1e3
        if i >= 2:
            wall.append(w)
            dev.append(ctx.tracks_time())
    # the C call alone: the binding's concatenation of the per-pair lists is not the library's
    pr, flat, counts = ctx._track_inputs(case.pairs, case.matches, args.min_length)
    rows = int(case.offsets[-1])
    track, offs, out = np.zeros(rows, np.int32), np.zeros(rows // 2 + 1, np.int64), np.zeros(rows, np.int32)
    call = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        T = sgpu.lib().sgpu_tracks_batch(ctx._ctx, case.offsets.ctypes.data, args.sets, pr.ctypes.data,
                                         len(pr), flat.ctypes.data, counts.ctypes.data, args.min_length,
                                         track.ctypes.data, offs.ctypes.data, out.ctypes.data, None)
        call.append((time.perf_counter() - t0) * 1e3)
        assert T == len(got.offsets) - 1
    ctx.close()
    with tempfile.TemporaryDirectory() as tmp:
        host, want = host_loop(case, args.min_length, args.repeats, tmp)
    assert np.array_equal(got.track_of_row, want.track) and np.array_equal(got.offsets, want.offsets)
    assert np.array_equal(got.rows, want.rows) and np.array_equal(got.stats, want.stats)
    res = {"workload": f"{args.sets} sets x {args.rows} rows, all {len(case.pairs)} pairs, {npoints} planted "
                       f"points, 70 % of the common points and 2 % wrong matches per pair; min_length "
                       f"{args.min_length}",
           "rows": rows, "matches": int(total), "upload_bytes": int(upload),
           "stats": [int(x) for x in got.stats], "track_rows": int(len(got.rows)),
           "device_ms": stats(dev), "c_call_wall_ms": stats(call), "binding_wall_ms": stats(wall),
           "host_loop_ms": stats(host),
           "host_loop_over_c_call_median": float(np.median(host) / np.median(call))}
    print(json.dumps(res), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"tracks_time_{args.tag}.json"), "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="run")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--rows", type=int, default=8000)
    ap.add_argument("--min-length", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=300, help="seconds for the GPU step")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
           "--child", "--tag", args.tag, "--repeats", str(args.repeats), "--sets", str(args.sets),
           "--rows", str(args.rows), "--min-length", str(args.min_length), "--out", args.out]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
