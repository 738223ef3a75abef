"""Extract the C3 shard (128 x 1080p) once, then time matching its 127 consecutive image pairs two
ways, alternating:

  (a) batched: SiftContext.match_images -- quantise in HBM, one grouped call (timed with the
      quantisation inside every call, and again with the u8 descriptors kept from the last call);
  (b) per pair, as before sgpu_match_images existed: features() download of both images' float
      descriptors, sgpu.quantize on the host, gpu_ctx.match.

It first asserts that both return identical pairs, then writes profiles/match_images_<tag>.json
with the medians and spreads: wall time of each way (a host clock around calls that end in a
synchronise), the batched call's device time (sgpu_last_timing's times[8]) and the sum of the
per-pair device times.

    python tests/match_images_time.py [--tag TAG] [--repeats 10] [--images 128]

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

    n = args.images
    imgs = synth_batch_fast(n, 1920, 1080, 3000)
    ctx = sgpu.SiftContext(0, default_options())
    ctx.extract(imgs)
    counts = [ctx.count(i) for i in range(n)]
    pairs = [(i, i + 1) for i in range(n - 1)]

    def batched(cached=False):
        if not cached:
            ctx.set_options(ctx.opts)   # drops the cached u8 descriptors: the call quantises again
        t0 = time.perf_counter()
        m = ctx.match_images(pairs)
        wall = (time.perf_counter() - t0) * 1e3
        return m, wall, ctx.timing()["match"]

    def per_pair():
        t0 = time.perf_counter()
        out, dev = [], 0.0
        for a, b in pairs:
            _, da = ctx.features(a)
            _, db = ctx.features(b)
            out.append(ctx.match(sgpu.quantize(da), sgpu.quantize(db)).copy())
            dev += ctx.timing()["match"]
        return out, (time.perf_counter() - t0) * 1e3, dev

    ma, _, _ = batched()
    mb, _, _ = per_pair()
    assert len(ma) == len(mb) == len(pairs)
    for p, (x, y) in enumerate(zip(ma, mb)):
        assert x.shape == y.shape and np.array_equal(x, y), f"pair {p}: results differ"
    print(f"identical pairs: {sum(len(x) for x in ma)} matches over {len(pairs)} pairs, "
          f"{sum(counts)} features", flush=True)
    for _ in range(2):   # warm-up of both (the first calls above allocated)
        batched()
        per_pair()
    wa, da, wc, dc, wb, db = [], [], [], [], [], []
    for _ in range(args.repeats):
        _, w, d = batched()
        wa.append(w)
        da.append(d)
        _, w, d = batched(cached=True)
        wc.append(w)
        dc.append(d)
        _, w, d = per_pair()
        wb.append(w)
        db.append(d)
    res = {
        "workload": f"C3 shard: {n} x 1920x1080 (synth_batch_fast seed 3000), "
                    f"{len(pairs)} consecutive pairs, mutual, distmax 0.7, ratiomax 0.8",
        "features_total": int(sum(counts)), "features_min": int(min(counts)),
        "features_max": int(max(counts)), "matches_total": int(sum(len(x) for x in ma)),
        "identical_pairs": True,
        # every call quantises the batch's descriptors again (the state after an extract) ...
        "batched_wall_ms": stats(wa), "batched_device_ms": stats(da),
        # ... and with the u8 descriptors kept from the previous call
        "batched_cached_wall_ms": stats(wc), "batched_cached_device_ms": stats(dc),
        "per_pair_wall_ms": stats(wb), "per_pair_device_sum_ms": stats(db),
        "wall_speedup_median": float(np.median(wb) / np.median(wa)),
    }
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"match_images_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    ctx.close()
    assert res["batched_wall_ms"]["median"] < res["per_pair_wall_ms"]["median"], \
        "the batched call is not faster than the per-pair flow"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="run")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--limit", type=int, default=540, help="seconds for the GPU step")
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
