"""Records tests/golden/ref_*.npz from the reference's own kernels run on the CPU
(oracle/_ref/libref_kernels.so, tests/ref_kernels.py), so that tests/test_ref_kernels.py pins the
oracle to them where no checkout of the reference is present.

The fixtures hold what the reference's programs write when run -- match lists, sign images,
filtered levels, oriented keys, descriptors -- for inputs that tests/ref_cases.py builds from
seeds; each stage ran on the oracle's output of the stage before it.
Run: python tests/make_ref_golden.py   (after build(), on a machine with the reference)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "modify-sift-gpu_amd", "python"))

import numpy as np  # noqa: E402

import oracle_py as O  # noqa: E402
import ref_cases as C  # noqa: E402
import ref_kernels as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def save(name, **arrays):
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, **arrays)
    print(name, os.path.getsize(path), "bytes")


def main():
    assert R.available(), R.SKIP_REASON
    out = {}
    for name in C.MATCH_SMALL:
        q1, q2, kw = C.match_case(name)
        for mbm in (0, 1):
            row, col, _ = R.match_stages(q1, q2, mbm=mbm, **kw)
            out[f"{name}_mbm{mbm}"] = R.pairs(row, col)
    for name in C.GUIDED_SMALL:
        q1, q2, l1, l2, H, F, kw = C.guided_case(name)
        out[f"guided_{name}"] = R.match(q1, q2, kw["distmax"], kw["ratiomax"], kw["mbm"], loc1=l1,
                                        loc2=l2, H=H, F=F, hdistmax=kw["hdistmax"],
                                        fdistmax=kw["fdistmax"])
    save("ref_match.npz", **out)

    out = {}
    for j in range(3):
        st = C.levels("checker8")[(0, j)]
        d = st["dog"]
        out[f"sign_{j}"] = R.key(d[0], d[1], d[2], st["tdog"], st["tedge"])[..., 0].astype(np.int8)
    save("ref_keys_checker8.npz", **out)

    img = C.unit_image(131, 37, 3 * 131 + 37)
    sigmas, widths, out = [], [], {}
    for sigma in C.filter_sigmas():   # one level per filter width
        w = len(R.filter_kernel(sigma))
        if w in widths:
            continue
        out[f"level_{len(widths)}"] = R.filter_image(img, sigma)
        sigmas.append(sigma)
        widths.append(w)
    save("ref_filter.npz", sigmas=np.array(sigmas, np.float32), widths=np.array(widths, np.int32),
         **out)

    out = {}
    feat, lvl = O.features_oct(C.image("synth_160x120"))
    for (o, j), st in C.levels("synth_160x120").items():
        out[f"oriented_{o}_{j}"] = R.orientation(st["list"], st["grad"], st["key"], st["sigma"],
                                                 st["sigma_step"])
        out[f"desc_{o}_{j}"] = R.descriptor(feat[lvl == o * 3 + j], st["grad"])
    save("ref_features_160x120.npz", **out)


if __name__ == "__main__":
    main()
