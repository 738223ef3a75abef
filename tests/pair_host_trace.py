"""The kernel launches of every entry point over the grouped pair matcher's shared host path
(csrc/sgpu_pairs.cpp), for comparing two builds of the library: each of the 14 entry points --
sgpu_match_batch / _images (+ _guided), sgpu_estimate_batch / _images (+ _refined), sgpu_verify_batch
/ _images, sgpu_select_top_scale_batch / _images, sgpu_prematch_batch / _images -- is called once on
the inputs of tests/pair_calls.py under rocprofv3 --kernel-trace (no counters in the same run), with
a one-row quantise between the calls as the marker that splits the trace.

    python tests/pair_host_trace.py --tag new                       # this tree's library
    SGPU_LIB_PATH=<other>/libsiftgpu.so python tests/pair_host_trace.py --tag parent
    python tests/pair_host_trace.py --compare parent new            # -> profiles/pair_host_trace.json

A run writes <out>/<tag>.json (--out, default build_exp/pair_host_trace): per entry point the
ordered list of (kernel, grid, workgroup).  A plain script, not a test; the GPU work runs in a child
process under a time limit."""
import argparse
import csv
import glob
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "modify-sift-gpu_amd", "python"))
OUT = os.path.join(ROOT, "build_exp", "pair_host_trace")


def entry_points():
    """(C entry point, f(ctx, putative of the sets, putative of the images)), in call order."""
    import pair_calls as PC
    buf, loc, scale, off, H = PC.sets()
    IP, IH, S, T = PC.IMAGE_PAIRS, PC.image_H(), PC.SEED, PC.TOP
    return [
        ("sgpu_match_batch", lambda c, P, Q: c.match_batch(buf, off, PC.PAIRS)),
        ("sgpu_match_batch_guided", lambda c, P, Q: c.match_batch_guided(buf, loc, off, PC.PAIRS, H=H)),
        ("sgpu_estimate_batch", lambda c, P, Q: c.estimate_batch(loc, off, PC.PAIRS, P, "H", seed=S)),
        ("sgpu_estimate_batch_refined",
         lambda c, P, Q: c.estimate_batch_refined(loc, off, PC.PAIRS, P, "F", 4.0, seed=S)),
        ("sgpu_verify_batch", lambda c, P, Q: c.verify_batch(buf, loc, off, PC.PAIRS, True, True, seed=S)),
        ("sgpu_select_top_scale_batch", lambda c, P, Q: c.select_top_scale(scale, off, T)),
        ("sgpu_prematch_batch", lambda c, P, Q: c.prematch_batch(buf, scale, off, PC.PAIRS, top=T)),
        ("sgpu_match_images", lambda c, P, Q: c.match_images(IP)),
        ("sgpu_match_images_guided", lambda c, P, Q: c.match_images_guided(IP, H=IH)),
        ("sgpu_estimate_images", lambda c, P, Q: c.estimate_images(IP, Q, "H", seed=S)),
        ("sgpu_estimate_images_refined",
         lambda c, P, Q: c.estimate_images_refined(IP, Q, "F", 4.0, seed=S)),
        ("sgpu_verify_images", lambda c, P, Q: c.verify_images(IP, True, True, seed=S)),
        ("sgpu_select_top_scale_images", lambda c, P, Q: c.select_top_scale_images(T)),
        ("sgpu_prematch_images", lambda c, P, Q: c.prematch_images(IP, top=T)),
    ]


def child():
    import numpy as np
    import pair_calls as PC
    import sgpu
    from sgpu_types import default_options
    ctx = sgpu.SiftContext(0, default_options())
    one = np.full((1, 128), 0.1, np.float32)
    marker = lambda: ctx.quantize_gpu(one)
    marker()   # the trace's first kernel: what a marker looks like
    ctx.extract(PC.views())
    marker()
    P = Q = None
    for name, f in entry_points():
        r = f(ctx, P, Q)
        marker()
        if name == "sgpu_match_batch":
            P = r
        if name == "sgpu_match_images":
            Q = r
    ctx.close()
    print("library", sgpu.LIB_PATH, flush=True)


def launches(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    short = lambda n: n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
    # the library's kernels: the runtime's own copy and fill kernels are left out
    return [[short(r["Kernel_Name"])] +
            [[int(r[f"{k}_Size_{a}"]) for a in "XYZ"] for k in ("Grid", "Workgroup")]
            for r in rows if not r["Kernel_Name"].startswith("__amd_rocclr")]


def run(tag, limit):
    out = os.path.join(OUT, tag)
    os.makedirs(out, exist_ok=True)
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--output-format", "csv",
           "-d", out, "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child"]
    rc = subprocess.run(cmd).returncode
    if rc != 0:   # nothing more is started on the GPU after a failed process
        return rc
    return split(tag)


def split(tag):
    out = os.path.join(OUT, tag)
    found = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    assert len(found) == 1, found
    trace = launches(found[0])
    marker, parts = trace[0], [[]]
    assert "k_quantize_desc" in marker[0], marker
    for rec in trace:
        if rec == marker:
            parts.append([])
        else:
            parts[-1].append(rec)
    names = [n for n, _ in entry_points()]
    # nothing, the extract, one part per entry point, nothing after the last marker
    assert len(parts) == len(names) + 3 and not parts[0] and not parts[-1], len(parts)
    res = {"library": os.environ.get("SGPU_LIB_PATH") or "in-tree", "marker": marker,
           "launches": sum(len(p) for p in parts[2:]),
           "entry_points": dict(zip(names, parts[2:-1]))}
    with open(os.path.join(OUT, f"{tag}.json"), "w") as f:
        json.dump(res, f)
    print(tag, {n: len(v) for n, v in res["entry_points"].items()}, flush=True)
    return 0


def compare(a, b):
    ra, rb = (json.load(open(os.path.join(OUT, f"{t}.json"))) for t in (a, b))
    digest = lambda v: hashlib.sha256(json.dumps(v).encode()).hexdigest()
    per = {n: {"launches": len(ra["entry_points"][n]),
               "identical": ra["entry_points"][n] == rb["entry_points"][n]} for n in ra["entry_points"]}
    res = {"what": "rocprofv3 --kernel-trace of tests/pair_host_trace.py on the parent commit's library "
                   "and on this tree's, one MI355X, each in a run of its own: per entry point the "
                   "ordered list of [kernel, grid, workgroup]",
           "identical": all(v["identical"] for v in per.values()) and
                        list(ra["entry_points"]) == list(rb["entry_points"]),
           "per_entry_point": per,
           a: {"sha256": digest(ra["entry_points"]), "launches": ra["launches"],
               "entry_points": ra["entry_points"]},
           b: {"sha256": digest(rb["entry_points"]), "launches": rb["launches"],
               "entry_points": rb["entry_points"]}}
    with open(os.path.join(ROOT, "profiles", "pair_host_trace.json"), "w") as f:
        json.dump(res, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("identical:", res["identical"], {n: v for n, v in per.items() if not v["identical"]})
    return 0 if res["identical"] else 1


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="new")
    ap.add_argument("--out", default=OUT, help="directory of the traces and the per-tag lists")
    ap.add_argument("--limit", type=int, default=150, help="seconds for the GPU step")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar="TAG")
    ap.add_argument("--split", action="store_true", help="only split the trace a run left behind")
    args = ap.parse_args()
    OUT = os.path.abspath(args.out)
    if args.child:
        child()
        return 0
    if args.compare:
        return compare(*args.compare)
    return split(args.tag) if args.split else run(args.tag, args.limit)


if __name__ == "__main__":
    sys.exit(main())
