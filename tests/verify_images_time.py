"""Time SiftContext.verify_images against the chain of separate calls it fuses.

Workload: extract the C3 shard (128 x 1080p) once, then verify its 127 consecutive image pairs --
putative matching, refined estimation (threshold 2 / 4, 512 hypotheses, 3 rounds), guided
matching -- two ways, alternating, for model H and for H + F:

  (a) fused: SiftContext.verify_images -- one call, one table upload, one result download;
  (b) chain: match_images -> estimate_images_refined (once per model) -> match_images_guided
      through the existing bindings: the putative matches and the matrices come down and go up
      again between the calls.  This is the baseline: what the library offered before.

It first asserts that both ways return identical bytes, then writes
profiles/verify_images_<tag>.json with median [min, max] of the wall times, of the fused call's
device time (sgpu_last_timing's times[13]) and of the sum of the chain's device times (times[8] +
times[12] per model + times[8]), and the per-pair counts.

    python tests/verify_images_time.py [--tag TAG] [--repeats 10] [--images 128]

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

H_THRESHOLD, F_THRESHOLD, ITERATIONS, SEED, ROUNDS = 2.0, 4.0, 512, 1, 3


def stats(v):
    import numpy as np
    a = np.asarray(v, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
            "n": int(len(a))}


def child(args):
    import numpy as np
    import sgpu
    from sgpu_types import default_options
    from sift_synth import synth_batch_fast

    def times(ctx):
        t = np.zeros(14, np.float32)
        sgpu.lib().sgpu_last_timing(ctx._ctx, t.ctypes.data, 14)
        return t

    ctx = sgpu.SiftContext(0, default_options())
    n = args.images
    ctx.extract(synth_batch_fast(n, 1920, 1080, 3000))
    pairs = [(i, i + 1) for i in range(n - 1)]
    mm = max(ctx.count(i) for i in range(n))
    res = {"workload": f"C3 shard: {n} x 1920x1080 (synth_batch_fast seed 3000), {len(pairs)} "
                       f"consecutive pairs; thresholds H {H_THRESHOLD:g} / F {F_THRESHOLD:g} (estimate "
                       f"and guided pass), {ITERATIONS} hypotheses, {ROUNDS} rounds, seed {SEED}",
           "features_total": int(ctx.total())}

    for label, want_f in (("H", False), ("H+F", True)):
        def fused():
            t0 = time.perf_counter()
            out = ctx.verify_images(pairs, True, want_f, max_match=mm, h_threshold=H_THRESHOLD,
                                    f_threshold=F_THRESHOLD, hdistmax=H_THRESHOLD,
                                    fdistmax=F_THRESHOLD, iterations=ITERATIONS, seed=SEED,
                                    refine_rounds=ROUNDS)
            return out, (time.perf_counter() - t0) * 1e3, float(times(ctx)[13])

        def chain():
            t0 = time.perf_counter()
            P = ctx.match_images(pairs, max_match=mm)
            dev = float(times(ctx)[8])
            Hm, iH, _, _ = ctx.estimate_images_refined(pairs, P, "H", H_THRESHOLD, ITERATIONS, SEED,
                                                       rounds=ROUNDS)
            dev += float(times(ctx)[12])
            Fm = iF = None
            if want_f:
                Fm, iF, _, _ = ctx.estimate_images_refined(pairs, P, "F", F_THRESHOLD, ITERATIONS,
                                                           SEED, rounds=ROUNDS)
                dev += float(times(ctx)[12])
            G = ctx.match_images_guided(pairs, Hm, Fm, hdistmax=H_THRESHOLD, fdistmax=F_THRESHOLD,
                                        max_match=mm)
            dev += float(times(ctx)[8])
            wall = (time.perf_counter() - t0) * 1e3
            return (G, Hm, iH, Fm, iF, np.array([len(m) for m in P], np.int32)), wall, dev

        a, b = fused()[0], chain()[0]
        assert a[5].tolist() == b[5].tolist(), "putative counts differ from the chain's"
        for k in (1, 3):
            assert (a[k] is None) == (b[k] is None)
            if a[k] is not None:
                assert a[k].tobytes() == b[k].tobytes(), "models differ from the chain's"
                assert a[k + 1].tolist() == b[k + 1].tolist()
        assert len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
        for _ in range(2):
            fused()
            chain()
        wf, df, wc, dc = [], [], [], []
        for _ in range(args.repeats):
            _, w, d = fused()
            wf.append(w)
            df.append(d)
            _, w, d = chain()
            wc.append(w)
            dc.append(d)
        res[label] = {
            "identical_bytes": True,
            "putative_total": int(a[5].sum()), "putative_median": float(np.median(a[5])),
            "verified_total": int(sum(len(m) for m in a[0])),
            "pairs_with_H": int((a[2] > 0).sum()),
            "pairs_with_F": int((a[4] > 0).sum()) if want_f else None,
            "fused_wall_ms": stats(wf), "chain_wall_ms": stats(wc),
            "fused_device_ms": stats(df), "chain_device_sum_ms": stats(dc),
            "chain_over_fused_wall_median": float(np.median(wc) / np.median(wf)),
            "fused_minus_chain_device_median_ms": float(np.median(df) - np.median(dc)),
            "chain_device_spread_ms": float(max(dc) - min(dc)),
        }
        print(label, json.dumps(res[label]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", f"verify_images_{args.tag}.json"), "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="run")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--limit", type=int, default=420, help="seconds for the GPU step")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
           "--child", "--tag", args.tag, "--repeats", str(args.repeats), "--images", str(args.images)]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
