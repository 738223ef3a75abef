"""The matcher's device-pointer forms (SGPU_INPUT_DEVICE): sgpu_match, sgpu_match_guided and
sgpu_quantize_descriptors_gpu on buffers the caller owns in device memory (devmem.py), against the
CPU oracle and the host-pointer calls."""
import numpy as np
import pytest

import devmem
import oracle_py as O
import sgpu
from sift_synth import synth_descriptors, synth_guided_scene

pytestmark = pytest.mark.gpu

N1, N2, SEED = 257, 1000, 23


def test_match_on_device_descriptors(gpu_ctx):
    q1, q2 = synth_guided_scene(N1, N2, SEED)[:2]
    want = O.match(q1, q2)
    assert len(want) > 0
    host = gpu_ctx.match(q1, q2).copy()
    with devmem.uploaded(q1) as p1, devmem.uploaded(q2) as p2:
        got = gpu_ctx.match(None, None, device_ptrs=(p1, N1, p2, N2)).copy()
        swapped = gpu_ctx.match(None, None, device_ptrs=(p2, N2, p1, N1)).copy()
    assert np.array_equal(got, want) and np.array_equal(got, host)
    assert np.array_equal(swapped, O.match(q2, q1))


@pytest.mark.parametrize("use", ["HF", "H", "F"])
def test_match_guided_on_device_buffers(gpu_ctx, use):
    q1, q2, l1, l2, H, F = synth_guided_scene(N1, N2, SEED)
    H = H if "H" in use else None
    F = F if "F" in use else None
    want = O.match_guided(q1, q2, l1, l2, H, F)
    assert len(want) > 0
    host = gpu_ctx.match_guided(q1, q2, l1, l2, H, F).copy()
    with devmem.uploaded(q1) as p1, devmem.uploaded(q2) as p2, \
            devmem.uploaded(l1) as g1, devmem.uploaded(l2) as g2:
        got = gpu_ctx.match_guided(None, None, None, None, H, F,
                                   device_ptrs=(p1, N1, p2, N2, g1, g2)).copy()
    assert np.array_equal(got, want) and np.array_equal(got, host)


def test_quantize_on_device_buffers(gpu_ctx):
    d = synth_descriptors(N2, SEED)
    # the quantiser's ends and its modulo-256 wrap (512 * 0.5 = 256)
    d[:4] = np.array([0.0, 1.0, 0.4990234, 0.5])[:, None]
    d = d.astype(np.float32)
    want = sgpu.quantize(d)
    with devmem.uploaded(d) as src, devmem.allocated(d.size) as out:
        out.upload(np.full(d.size, 0xA5, np.uint8))
        assert gpu_ctx.quantize_gpu(None, device_ptrs=(src, len(d), out.base)) is None
        got = out.download(d.shape, np.uint8)
    assert np.array_equal(got, want)
    assert np.array_equal(gpu_ctx.quantize_gpu(d), want)
