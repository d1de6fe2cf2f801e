"""Writes tests/golden/golden_denoise_spatial_v1.npz: the inputs, the parameters and the outputs of the spatial top-up's definition
(tests/denoise_spatial_spec_numpy.py) on tests/denoise_spatial_cases.golden_cases -- image, mask, weight (an empty array: none), [strength, target,
search] as the case has them (0: the default), and the definition's image, support and [unset, kept, smoothed]; tests/test_denoise_spatial_cpu.py
recomputes them.  Run from the repository root:
    python tests/golden/make_golden_denoise_spatial.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import denoise_spatial_cases as cases  # noqa: E402


def main():
    out = {}
    for case in cases.golden_cases():
        r = cases.run_spec(case)
        n = case["name"] + "/"
        out.update({n + "in_image": case["image"], n + "in_mask": case["mask"], n + "in_weight": case["weight"] if case["weight"] is not None else np.zeros(0, dtype=np.uint8),
                    n + "params": np.array([case["strength"], case["target"], case["search"]], dtype=np.int64), n + "image": r["image"], n + "support": r["support"],
                    n + "counts": np.array(r["counts"], dtype=np.int64)})
        print(case["name"], "weight" if case["weight"] is not None else "no weight", "h", case["strength"], "target", case["target"], "[unset, kept, smoothed]", r["counts"],
              "support", int(r["support"].min()), "..", int(r["support"].max()))
    path = os.path.join(HERE, "golden_denoise_spatial_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
