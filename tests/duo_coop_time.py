"""In-process A/B of the paired Gaussian's strip geometry on bench.py's step:
the per-wave strips (STRIPS_WAVE), the shipped rule (STRIPS_RULE) and the cooperative strips
wherever compiled (STRIPS_COOP), switched by sgpu_debug_set_duo_strips in one context over the same
staged batch, alternating, `rounds` times `steps` steps each; prints one JSON line with every
round's pyramid stage time (HIP events around the pyramid's launches, ms per step) and wall time
per step.

  python tests/duo_coop_time.py [--rounds 5] [--steps 10] [--batch 128] [--width 1920]
                                [--height 1080] [--octaves 4]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "modify-sift-gpu_amd", "python"))

import sgpu  # noqa: E402
from sgpu_types import default_options  # noqa: E402
from sift_synth import synth_batch_fast  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--octaves", type=int, default=4)
    args = ap.parse_args()
    ctx = sgpu.SiftContext(0, default_options(octave_num=args.octaves))
    ctx.stage(synth_batch_fast(args.batch, args.width, args.height, 3000))
    modes = [("wave", ctx.STRIPS_WAVE), ("rule", ctx.STRIPS_RULE), ("coop", ctx.STRIPS_COOP)]
    for _, m in modes:   # warm-up: every form's kernels loaded, buffers sized
        ctx.set_duo_strips(m)
        for _ in range(3):
            ctx.extract_staged()
    runs = {name: [] for name, _ in modes}
    for _ in range(args.rounds):
        for name, m in modes:
            ctx.set_duo_strips(m)
            ctx.extract_staged()
            pyr = 0.0
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ctx.extract_staged()
                pyr += ctx.timing()["pyramid"]
            wall = time.perf_counter() - t0
            runs[name].append({"pyramid_ms": pyr / args.steps, "ms_per_step": wall / args.steps * 1e3})
    ctx.set_duo_strips(ctx.STRIPS_RULE)
    ctx.close()
    print(json.dumps({"workload": vars(args), "runs": runs}))


if __name__ == "__main__":
    main()
