"""Time SiftContext.estimate_images / estimate_batch against the host flow they replace.

Row 1: extract the C3 shard (128 x 1080p) once, match its 127 consecutive image pairs with
SiftContext.match_images, then estimate one H per pair (threshold 2, 512 hypotheses) two ways,
alternating:

  (a) device: SiftContext.estimate_images -- one call, the keys stay in HBM;
  (b) host: download every image's keys (features()), then sgeo::estimate_host of
      csrc/sift_geom.h, single-threaded, g++ -O2 (tests/abi/geom_check.cpp in file mode; its own
      clock around the loop, so neither the process start nor the file I/O counts).

The shard's images are independent, so a pair has only a few dozen putative matches and the work
per pair is small.  Row 2 is where the hypothesis x match product is large: a synthetic list of
1,000 pairs of 1,000 matches each (planted H scenes of geom_scenes.h_scene), estimate_batch
against estimate_host.

It first asserts that both ways return identical bytes, then writes
profiles/estimate_images_<tag>.json with median [min, max] of the wall times and of the call's
device time (sgpu_last_timing's times[12]), and the per-pair match counts.

    python tests/estimate_images_time.py [--tag TAG] [--repeats 10] [--images 128]

A plain script, not a test.  The GPU work runs in a child process under a time limit."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "modify-sift-gpu_amd", "python"))

THRESHOLD, ITERATIONS, SEED = 2.0, 512, 1


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

    exe = G.check_program(False)

    def times12(ctx):
        t = np.zeros(13, np.float32)
        sgpu.lib().sgpu_last_timing(ctx._ctx, t.ctypes.data, 13)
        return float(t[12])

    def host_run(d):
        """estimate_host on the scene in d: (models, inliers, mask bytes, its own clock in ms)."""
        r = subprocess.run([exe, "run", d], capture_output=True, text=True, check=True)
        ms = [float(l.split()[1]) for l in r.stdout.splitlines() if l.startswith("host_ms")]
        return (np.fromfile(os.path.join(d, "models.bin"), np.float32),
                np.fromfile(os.path.join(d, "inliers.bin"), np.int32),
                np.fromfile(os.path.join(d, "mask.bin"), np.uint8), ms[0])

    def compare(dev, host):
        models, inliers, masks = dev
        hm, hi, hk, _ = host
        assert models.tobytes() == hm.tobytes(), "models differ from the host's"
        assert np.array_equal(inliers, hi) and np.array_equal(np.concatenate(masks).astype(np.uint8), hk)

    res = {}
    ctx = sgpu.SiftContext(0, default_options())

    # ---- row 1: the shard ----
    n = args.images
    ctx.extract(synth_batch_fast(n, 1920, 1080, 3000))
    pairs = [(i, i + 1) for i in range(n - 1)]
    putative = ctx.match_images(pairs)
    mcounts = [len(m) for m in putative]

    def device_images():
        t0 = time.perf_counter()
        out = ctx.estimate_images(pairs, putative, "H", THRESHOLD, ITERATIONS, SEED)
        return out, (time.perf_counter() - t0) * 1e3, times12(ctx)

    def download():
        t0 = time.perf_counter()
        keys = [ctx.features(i, descriptors=False)[0] for i in range(n)]
        return keys, (time.perf_counter() - t0) * 1e3

    with tempfile.TemporaryDirectory(prefix="estimate_time_") as d:
        keys, _ = download()
        off = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)
        loc = np.concatenate([k[:, :2] for k in keys])
        G.write_scene(d, loc, off, pairs, putative, "H", THRESHOLD, ITERATIONS, SEED)
        compare(device_images()[0], host_run(d))
        for _ in range(2):
            device_images()
        wd, dd, wk, hh = [], [], [], []
        for _ in range(args.repeats):
            out, w, t = device_images()
            wd.append(w)
            dd.append(t)
            wk.append(download()[1])
            hh.append(host_run(d)[3])
        inl = out[1]
    res["shard"] = {
        "workload": f"C3 shard: {n} x 1920x1080 (synth_batch_fast seed 3000), {len(pairs)} "
                    f"consecutive pairs after match_images; H, threshold {THRESHOLD:g}, "
                    f"{ITERATIONS} hypotheses",
        "matches_total": int(sum(mcounts)), "matches_min": int(min(mcounts)),
        "matches_median": float(np.median(mcounts)), "matches_max": int(max(mcounts)),
        "pairs_with_model": int((inl > 0).sum()), "inliers_median": float(np.median(inl)),
        "identical_bytes": True,
        "device_wall_ms": stats(wd), "device_ms": stats(dd),
        "host_key_download_wall_ms": stats(wk), "host_estimate_ms": stats(hh),
        "host_over_device_wall_median": float((np.median(wk) + np.median(hh)) / np.median(wd)),
    }
    print(json.dumps(res["shard"]), flush=True)

    # ---- row 2: 1,000 pairs x 1,000 matches ----
    nsc, npairs, m = 20, args.synthetic_pairs, 1000
    sets, ms = [], []
    for s in range(nsc):
        la, lb, mt, _ = G.h_scene(seed=900 + s, n=m, n_planted=600)
        sets += [la, lb]
        ms.append(mt)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    loc = np.concatenate(sets)
    spairs = [(2 * (p % nsc), 2 * (p % nsc) + 1) for p in range(npairs)]
    smatches = [ms[p % nsc] for p in range(npairs)]

    def device_batch():
        t0 = time.perf_counter()
        out = ctx.estimate_batch(loc, off, spairs, smatches, "H", THRESHOLD, ITERATIONS, SEED)
        return out, (time.perf_counter() - t0) * 1e3, times12(ctx)

    with tempfile.TemporaryDirectory(prefix="estimate_time_") as d:
        G.write_scene(d, loc, off, spairs, smatches, "H", THRESHOLD, ITERATIONS, SEED)
        compare(device_batch()[0], host_run(d))
        device_batch()
        wd, dd, hh = [], [], []
        for r in range(args.repeats):
            out, w, t = device_batch()
            wd.append(w)
            dd.append(t)
            if r < args.host_repeats:
                hh.append(host_run(d)[3])
    res["synthetic"] = {
        "workload": f"{npairs} pairs x {m} matches (600 planted), H, threshold {THRESHOLD:g}, "
                    f"{ITERATIONS} hypotheses: {npairs * m * ITERATIONS:.3g} inlier tests",
        "inliers_median": float(np.median(out[1])), "identical_bytes": True,
        "device_wall_ms": stats(wd), "device_ms": stats(dd), "host_estimate_ms": stats(hh),
        "host_over_device_wall_median": float(np.median(hh) / np.median(wd)),
        "inlier_tests_per_second_device": float(npairs * m * ITERATIONS / (np.median(dd) * 1e-3)),
    }
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"estimate_images_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["synthetic"]), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="run")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=3, help="host runs of the synthetic row")
    ap.add_argument("--synthetic-pairs", type=int, default=1000)
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--limit", type=int, default=540, help="seconds for the GPU step")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return 0
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
           "--child", "--tag", args.tag, "--repeats", str(args.repeats), "--images", str(args.images),
           "--host-repeats", str(args.host_repeats), "--synthetic-pairs", str(args.synthetic_pairs)]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
