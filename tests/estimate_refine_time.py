"""Time the estimator's local refinement: the device time (sgpu_last_timing's times[12]) of
SiftContext.estimate_images and of estimate_images_refined at rounds 0 and 3, on the two pair
lists of tests/estimate_images_time.py:

  shard      extract the C3 shard (128 x 1080p) once, match its 127 consecutive image pairs;
             one H per pair, threshold 2, 512 hypotheses;
  synthetic  1,000 pairs of 1,000 matches each (planted H scenes), estimate_batch[_refined].

Three alternating runs, each a fresh process per build: --parent (the modify-sift-gpu_amd directory
of a built checkout of the parent commit, which has only the unrefined call: its lib/ and its
python/ binding are used) when given, then this tree's build.  rounds
= 0 issues the unrefined call's launches, so its time belongs inside the unrefined call's own
run-to-run spread; the cost of rounds = 3 is what the added launch takes.  It first asserts that
rounds = 0 returns the unrefined bytes and that no refined count is lower, then writes
profiles/estimate_refine_<tag>.json with median [min, max] per run and variant.

    python tests/estimate_refine_time.py [--tag TAG] [--repeats 10] [--images 128] [--parent DIR]

A plain script, not a test.  The GPU work runs in child processes, each under a time limit."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
# (a child of the parent build finds that build's binding through PYTHONPATH, ahead of this one)
sys.path.append(os.path.join(ROOT, "modify-sift-gpu_amd", "python"))

THRESHOLD, ITERATIONS, SEED, ROUNDS = 2.0, 512, 1, 3


def stats(v):
    import numpy as np
    a = np.asarray(v, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
            "n": int(len(a))}


def child(args):
    import numpy as np
    import geom_scenes as G
    import sgpu
    from sgpu_types import default_options
    from sift_synth import synth_batch_fast

    def times12(ctx):
        t = np.zeros(13, np.float32)
        sgpu.lib().sgpu_last_timing(ctx._ctx, t.ctypes.data, 13)
        return float(t[12])

    refined = hasattr(sgpu.SiftContext, "estimate_batch_refined")
    ctx = sgpu.SiftContext(0, default_options())
    n = args.images
    ctx.extract(synth_batch_fast(n, 1920, 1080, 3000))
    pairs = [(i, i + 1) for i in range(n - 1)]
    putative = ctx.match_images(pairs)
    nsc, m = 20, 1000
    sets, ms = [], []
    for s in range(nsc):
        la, lb, mt, _ = G.h_scene(seed=900 + s, n=m, n_planted=600)
        sets += [la, lb]
        ms.append(mt)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    loc = np.concatenate(sets)
    spairs = [(2 * (p % nsc), 2 * (p % nsc) + 1) for p in range(args.synthetic_pairs)]
    smatches = [ms[p % nsc] for p in range(args.synthetic_pairs)]
    case = ("H", THRESHOLD, ITERATIONS, SEED)
    calls = {
        "shard": {"plain": lambda: ctx.estimate_images(pairs, putative, *case)},
        "synthetic": {"plain": lambda: ctx.estimate_batch(loc, off, spairs, smatches, *case)},
    }
    if refined:
        for r in (0, ROUNDS):
            calls["shard"][f"rounds{r}"] = lambda r=r: ctx.estimate_images_refined(pairs, putative, *case, rounds=r)
            calls["synthetic"][f"rounds{r}"] = lambda r=r: ctx.estimate_batch_refined(loc, off, spairs, smatches, *case, rounds=r)
    res = {}
    for row, variants in calls.items():
        out = {k: f() for k, f in variants.items()}   # (also the warm-up)
        res[row] = {"times": {k: [] for k in variants}}
        if refined:
            plain, zero, more = out["plain"], out["rounds0"], out[f"rounds{ROUNDS}"]
            assert zero[0].tobytes() == plain[0].tobytes() and np.array_equal(zero[1], plain[1])
            assert not zero[3].any() and (more[1] >= plain[1]).all()
            res[row].update(pairs=len(plain[1]), pairs_refined=int((more[3] > 0).sum()),
                            rounds_mean=float(more[3].mean()),
                            inliers_plain=int(plain[1].sum()), inliers_refined=int(more[1].sum()))
        for _ in range(args.repeats):
            for k, f in variants.items():   # alternating
                f()
                res[row]["times"][k].append(times12(ctx))
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="run")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--synthetic-pairs", type=int, default=1000)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--limit", type=int, default=150, help="seconds for each GPU process")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
           "--child", "--repeats", str(args.repeats), "--images", str(args.images),
           "--synthetic-pairs", str(args.synthetic_pairs)]
    libs = ([("parent", args.parent)] if args.parent else []) + [("this", None)]
    res = {"workload": f"H, threshold {THRESHOLD:g}, {ITERATIONS} hypotheses; shard: {args.images} x "
                       f"1920x1080, consecutive pairs; synthetic: {args.synthetic_pairs} pairs x 1000 "
                       f"matches; times[12] in ms, {args.repeats} alternating repeats per run",
           "runs": []}
    for run in range(args.runs):
        entry = {}
        for name, path in libs:
            env = dict(os.environ)
            if path:
                env["SGPU_LIB_PATH"] = os.path.join(os.path.abspath(path), "lib", "libsiftgpu.so")
                env["PYTHONPATH"] = os.path.join(os.path.abspath(path), "python")
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:   # nothing more is started on the GPU after a failed process
                sys.stderr.write(r.stdout + r.stderr)
                return r.returncode
            got = json.loads(r.stdout.split("RESULT ", 1)[1])
            for row, v in got.items():
                e = entry.setdefault(row, {})
                e.update({k: x for k, x in v.items() if k != "times"})
                for k, t in v["times"].items():
                    e[f"{name}_{k}_ms"] = stats(t)
        res["runs"].append(entry)
        print(json.dumps(entry), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", f"estimate_refine_{args.tag}.json"), "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
