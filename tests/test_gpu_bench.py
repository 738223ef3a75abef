"""bench.py as a program: a plain run times exactly --steps steps, carries only the headline's
fields, and --dump-outputs writes the last timed step's features -- the ones an extraction of
the same seeded batch gives in this process, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sgpu_types import default_options
from sift_synth import synth_batch_fast

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, W, H = 3, 320, 240


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_plain_run_is_the_headline_and_dumps_the_last_step(gpu_ctx, tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--batch", str(B), "--width", str(W), "--height", str(H),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "images/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["ms_per_step"] > 0
    # images/s and ms_per_step describe the same two timed steps
    assert line["value"] == pytest.approx(B / (line["ms_per_step"] * 1e-3), rel=1e-9)
    # what --full adds is not run
    for k in ("c2", "c4", "match", "end_to_end", "cpu_baseline", "verify"):
        assert k not in line, k

    got = {n[:-4]: np.load(out / n) for n in sorted(os.listdir(out))}
    assert sorted(got) == ["counts", "descriptor_images", "descriptors", "keys"]
    assert got["counts"].dtype == np.float64 and got["descriptor_images"].dtype == np.float64
    assert got["keys"].dtype == np.float32 and got["descriptors"].dtype == np.float32
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    # the bench's inputs are the seeded batch; the same batch here gives the same features
    opts = default_options(octave_num=4)
    gpu_ctx.set_options(opts)
    try:
        gpu_ctx.extract(synth_batch_fast(B, W, H, 3000))
        feats = [gpu_ctx.features(i) for i in range(B)]
    finally:
        gpu_ctx.set_options(default_options())
    counts = np.array([len(k) for k, _ in feats], np.float64)
    assert counts.min() > 0
    assert np.array_equal(got["counts"], counts)
    assert np.array_equal(_bits(got["keys"]), _bits(np.concatenate([k for k, _ in feats])))
    picked = got["descriptor_images"].astype(int).tolist()
    assert sorted(picked) == list(range(B))   # everything fits at this size
    assert np.array_equal(_bits(got["descriptors"]),
                          _bits(np.concatenate([feats[i][1] for i in picked])))
