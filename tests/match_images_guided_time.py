"""Extract the C3 shard (128 x 1080p) once, match its 127 consecutive image pairs with
SiftContext.match_images (the putative pass), then time the guided second pass two ways,
alternating:

  (a) grouped: SiftContext.match_images_guided -- one call, descriptors and keys stay in HBM;
  (b) per pair, the flow without the grouped guided call: features() download of both images'
      keys and float descriptors, sgpu.quantize on the host, gpu_ctx.match_guided.

The geometry is a fixed rule, no estimation: H = identity for every pair with hdistmax = 200
pixels (a match may move at most 200 px in x and in y between consecutive images), no F.  The
shard's images are independent, so the rule decides a lot: it removes matches and, more often,
the rivals that kept a row from passing the ratio test (more matches than the putative pass).

It first asserts that both ways return identical pairs, then writes
profiles/match_images_guided_<tag>.json with the medians and spreads: wall time of each way (a
host clock around calls that end in a synchronise), the grouped call's device time
(sgpu_last_timing's times[8]) next to the plain match_images device time on the same pairs (what
the fused geometric test costs), and the sum of the per-pair device times.

    python tests/match_images_guided_time.py [--tag TAG] [--repeats 10] [--images 128]

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

HDISTMAX = 200.0


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
    H = np.tile(np.eye(3, dtype=np.float32), (len(pairs), 1, 1))
    eye = np.eye(3, dtype=np.float32)

    def plain():
        t0 = time.perf_counter()
        m = ctx.match_images(pairs)
        return m, (time.perf_counter() - t0) * 1e3, ctx.timing()["match"]

    def grouped():
        t0 = time.perf_counter()
        m = ctx.match_images_guided(pairs, H, None, hdistmax=HDISTMAX)
        return m, (time.perf_counter() - t0) * 1e3, ctx.timing()["match"]

    def per_pair():
        t0 = time.perf_counter()
        out, dev = [], 0.0
        for a, b in pairs:
            ka, da = ctx.features(a)
            kb, db = ctx.features(b)
            out.append(ctx.match_guided(sgpu.quantize(da), sgpu.quantize(db), ka[:, :2], kb[:, :2],
                                        eye, None, hdistmax=HDISTMAX).copy())
            dev += ctx.timing()["match"]
        return out, (time.perf_counter() - t0) * 1e3, dev

    putative, _, _ = plain()   # (also quantises the batch: every timed call finds the u8 forms)
    ma, _, _ = grouped()
    mb, _, _ = per_pair()
    assert len(ma) == len(mb) == len(pairs)
    for p, (x, y) in enumerate(zip(ma, mb)):
        assert x.shape == y.shape and np.array_equal(x, y), f"pair {p}: results differ"
    nput, ngui = sum(len(x) for x in putative), sum(len(x) for x in ma)
    print(f"identical pairs: {ngui} guided matches ({nput} putative) over {len(pairs)} pairs, "
          f"{sum(counts)} features", flush=True)
    for _ in range(2):   # warm-up of all three (the first calls above allocated)
        plain()
        grouped()
        per_pair()
    wp, dp, wa, da, wb, db = [], [], [], [], [], []
    for _ in range(args.repeats):
        _, w, d = plain()
        wp.append(w)
        dp.append(d)
        _, w, d = grouped()
        wa.append(w)
        da.append(d)
        _, w, d = per_pair()
        wb.append(w)
        db.append(d)
    res = {
        "workload": f"C3 shard: {n} x 1920x1080 (synth_batch_fast seed 3000), "
                    f"{len(pairs)} consecutive pairs, mutual, distmax 0.7, ratiomax 0.8; "
                    f"guided pass: H = identity, hdistmax {HDISTMAX:g}, no F",
        "features_total": int(sum(counts)), "features_min": int(min(counts)),
        "features_max": int(max(counts)), "putative_matches_total": int(nput),
        "guided_matches_total": int(ngui), "identical_pairs": True,
        "grouped_wall_ms": stats(wa), "grouped_device_ms": stats(da),
        # the plain grouped call on the same pairs, u8 descriptors cached as for the guided call
        "plain_wall_ms": stats(wp), "plain_device_ms": stats(dp),
        "per_pair_wall_ms": stats(wb), "per_pair_device_sum_ms": stats(db),
        "wall_speedup_median": float(np.median(wb) / np.median(wa)),
        "guided_over_plain_device_median": float(np.median(da) / np.median(dp)),
    }
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"match_images_guided_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)
    ctx.close()
    assert res["grouped_wall_ms"]["median"] < res["per_pair_wall_ms"]["median"], \
        "the grouped guided call is not faster than the per-pair flow"


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
