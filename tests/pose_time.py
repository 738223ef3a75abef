"""Time SiftContext.pose_batch against the host loop of the same rule.

Workload: 4,000 pairs of 300 matches each, over 8 two-view scenes of pose_scenes (the planted
motion, 70 % planted matches with +-0.3 px of noise, 30 % random ones, two different cameras), every
pair under the planted F at f_threshold 4 and min_angle 5 degrees, points and masks asked for.  The
same input goes two ways:

  (a) device: SiftContext.pose_batch -- sgpu_last_timing's times[16] (device: memset, gather and
      k_pose) and the wall time of the C call, upload and download included;
  (b) host: spose::pose_host through the stand-alone program tests/abi/pose_check.cpp, built here
      with g++ -O2, one thread, which times the loop alone (no file reading).

It checks that both give the same bytes and writes <out>/pose_time_<tag>.json with median
[min, max] of the times and the counts.

    python tests/pose_time.py [--tag TAG] [--repeats 10] [--pairs 4000] [--matches 300] [--out DIR]

A plain script, not a test.  The GPU work runs in a child process under a time limit."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "modify-sift-gpu_amd", "python"))

SCENES = 8


def stats(v):
    import numpy as np
    a = np.asarray(v, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
            "n": int(len(a))}


def workload(npairs, m):
    import numpy as np
    import pose_scenes as S
    scenes = [S.scene(seed=900 + i, n=m, n_planted=(7 * m) // 10, noise=0.3) for i in range(SCENES)]
    loc = np.concatenate([x for s in scenes for x in (s.la, s.lb)])
    off = np.arange(2 * SCENES + 1, dtype=np.int64) * m
    K = np.array([S.KA, S.KB] * SCENES, np.float32)
    pairs = [(2 * (p % SCENES), 2 * (p % SCENES) + 1) for p in range(npairs)]
    matches = [scenes[p % SCENES].matches for p in range(npairs)]
    return S.PairList(loc, off, K, pairs, matches, np.stack([S.F0] * npairs))


def child(args):
    import numpy as np
    import pose_scenes as S
    import sgpu
    pl = workload(args.pairs, args.matches)
    ctx = sgpu.SiftContext(0)
    wall, dev = [], []
    got = None
    for i in range(2 + args.repeats):
        t0 = time.perf_counter()
        got = ctx.pose_batch(pl.loc, pl.off, pl.pairs, pl.matches, pl.F, pl.K, S.THRESHOLD, S.MIN_ANGLE)
        w = (time.perf_counter() - t0) * 1e3
        if i >= 2:
            wall.append(w)
            dev.append(ctx.pose_time())
    # the C call alone: the binding's concatenation of the per-pair lists is not the library's
    off, nsets, lc, ptr, flags = ctx._estimate_sets(pl.loc, pl.off, None)
    pr, flat, counts, fm, km = ctx._pose_inputs(pl.pairs, pl.matches, pl.F, pl.K, nsets, S.THRESHOLD,
                                                S.MIN_ANGLE)
    R, t = np.zeros((len(pr), 9), np.float32), np.zeros((len(pr), 3), np.float32)
    oc = np.zeros((len(pr), 3), np.int32)
    mask, pts = np.zeros(len(flat), np.uint8), np.zeros((len(flat), 3), np.float32)
    call = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        rc = sgpu.lib().sgpu_pose_batch(ctx._ctx, ptr, off.ctypes.data, nsets, km.ctypes.data,
                                        pr.ctypes.data, len(pr), flat.ctypes.data, counts.ctypes.data,
                                        fm.ctypes.data, S.THRESHOLD, S.MIN_ANGLE, R.ctypes.data,
                                        t.ctypes.data, oc.ctypes.data, mask.ctypes.data, pts.ctypes.data,
                                        flags)
        call.append((time.perf_counter() - t0) * 1e3)
        assert rc == sgpu.SGPU_OK
    ctx.close()
    host = []
    want = S.host_pose(*pl, reps=args.repeats, times=host)
    assert len(host) == args.repeats
    assert got.R.tobytes() == want.R.tobytes() and got.t.tobytes() == want.t.tobytes()
    assert got.front.tolist() == want.front.tolist() and got.wide.tolist() == want.wide.tolist()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got.points, want.points))
    assert all(np.array_equal(a, b) for a, b in zip(got.masks, want.masks))
    res = {"workload": f"{args.pairs} pairs x {args.matches} matches over {SCENES} two-view scenes, 70 % "
                       f"planted matches with 0.3 px noise, the planted F, f_threshold {S.THRESHOLD}, "
                       f"min_angle 5 degrees, masks and points",
           "matches": int(len(flat)), "participants": int(got.participants.sum()),
           "front": int(got.front.sum()), "wide": int(got.wide.sum()),
           "device_ms": stats(dev), "c_call_wall_ms": stats(call), "binding_wall_ms": stats(wall),
           "host_loop_ms": stats(host),
           "host_loop_over_c_call_median": float(np.median(host) / np.median(call))}
    print(json.dumps(res), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"pose_time_{args.tag}.json"), "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="run")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=4000)
    ap.add_argument("--matches", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=300, help="seconds for the GPU step")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
           "--child", "--tag", args.tag, "--repeats", str(args.repeats), "--pairs", str(args.pairs),
           "--matches", str(args.matches), "--out", args.out]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
