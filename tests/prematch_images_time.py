"""Time SiftContext.prematch_images against full matching of the same pairs.

Workload: extract the C3 shard (128 x 1080p) once, then look at all 8,128 image pairs two ways,
alternating in one process:

  (a) pre-pass: SiftContext.prematch_images over all pairs with top = 100 -- every image's 100
      largest-scale features selected and gathered on the device, the pairs matched on those
      subsets -- counts only, and with the matches;
  (b) baseline: match_images over the same 8,128 pairs on the full feature sets: what the library
      offered before for "which pairs overlap?".

It writes <out>/prematch_images_<tag>.json with median [min, max] of the wall times (host clock)
and of the device times (sgpu_last_timing's times[14] for the pre-pass, times[8] for the baseline),
and how many of the baseline's pairs with at least 4 full matches the pre-pass keeps at 4 subset
matches.  The shard's images are independent scenes, so that last number mostly shows chance
matches being dropped, not overlap being found.

    python tests/prematch_images_time.py [--tag TAG] [--repeats 10] [--images 128] [--out DIR]
    python tests/prematch_images_time.py --kernels     # a few pre-pass calls only, for a
                                                       # kernel trace of the process

A plain script, not a test.  The GPU work runs in a child process under a time limit (--kernels
runs in this process, so that a profiler that starts it sees the kernels)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "modify-sift-gpu_amd", "python"))

TOP, MIN_MATCHES = 100, 4


def stats(v):
    import numpy as np
    a = np.asarray(v, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()),
            "n": int(len(a))}


def extracted(n):
    import sgpu
    from sgpu_types import default_options
    from sift_synth import synth_batch_fast
    ctx = sgpu.SiftContext(0, default_options())
    ctx.extract(synth_batch_fast(n, 1920, 1080, 3000))
    return ctx


def kernels(args):
    ctx = extracted(args.images)
    for _ in range(1 + args.repeats):
        ctx.prematch_images(None, TOP, matches=False)
    print("prematch device ms", ctx.prematch_time(), flush=True)
    ctx.close()


def child(args):
    import numpy as np
    import sgpu

    def times(ctx):
        t = np.zeros(15, np.float32)
        sgpu.lib().sgpu_last_timing(ctx._ctx, t.ctypes.data, 15)
        return t

    ctx = extracted(args.images)
    n = args.images
    a, b = np.triu_indices(n, 1)
    pairs = np.stack([a, b], axis=1).astype(np.int32)
    sizes = np.array([ctx.count(i) for i in range(n)])
    res = {"workload": f"C3 shard: {n} x 1920x1080 (synth_batch_fast seed 3000), all {len(pairs)} "
                       f"pairs; pre-pass top {TOP}; baseline match_images on the full sets",
           "features_total": int(ctx.total()), "features_per_image_median": float(np.median(sizes))}

    def pre(matches):
        t0 = time.perf_counter()
        out = ctx.prematch_images(None, TOP, matches=matches)
        return out, (time.perf_counter() - t0) * 1e3, float(times(ctx)[14])

    def base():
        t0 = time.perf_counter()
        out = ctx.match_images(pairs)
        return out, (time.perf_counter() - t0) * 1e3, float(times(ctx)[8])

    (pc, pm), (pc2, _), full = pre(True)[0], pre(False)[0], base()[0]
    assert pc.tolist() == pc2.tolist() == [len(m) for m in pm]
    fc = np.array([len(m) for m in full])
    for _ in range(2):
        pre(False)
        pre(True)
        base()
    acc = {k: [] for k in ("cw", "cd", "mw", "md", "bw", "bd")}
    for _ in range(args.repeats):
        for key, run in (("c", lambda: pre(False)), ("m", lambda: pre(True)), ("b", base)):
            _, w, d = run()
            acc[key + "w"].append(w)
            acc[key + "d"].append(d)
    base_keep, pre_keep = fc >= MIN_MATCHES, pc >= MIN_MATCHES
    res.update({
        "prematch_counts_wall_ms": stats(acc["cw"]), "prematch_counts_device_ms": stats(acc["cd"]),
        "prematch_matches_wall_ms": stats(acc["mw"]), "prematch_matches_device_ms": stats(acc["md"]),
        "baseline_wall_ms": stats(acc["bw"]), "baseline_device_ms": stats(acc["bd"]),
        "baseline_over_prematch_counts_wall_median": float(np.median(acc["bw"]) / np.median(acc["cw"])),
        "baseline_over_prematch_counts_device_median": float(np.median(acc["bd"]) / np.median(acc["cd"])),
        "prematch_matches_total": int(pc.sum()), "prematch_count_max": int(pc.max()),
        "baseline_matches_total": int(fc.sum()), "baseline_count_max": int(fc.max()),
        "baseline_pairs_with_min_matches": int(base_keep.sum()),
        "prematch_pairs_with_min_matches": int(pre_keep.sum()),
        "baseline_pairs_kept_by_prematch": int((base_keep & pre_keep).sum()),
        "fraction_of_baseline_pairs_kept": (float((base_keep & pre_keep).sum() / base_keep.sum())
                                            if base_keep.any() else None),
    })
    print(json.dumps(res), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"prematch_images_{args.tag}.json"), "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="run")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--limit", type=int, default=420, help="seconds for the GPU step")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    if args.kernels:
        kernels(args)
        return 0
    if args.child:
        child(args)
        return 0
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
           "--child", "--tag", args.tag, "--repeats", str(args.repeats), "--images", str(args.images),
           "--out", args.out]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
