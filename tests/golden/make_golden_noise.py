"""Writes tests/golden/golden_noise_v1.npz: the inputs, the quantile and the outputs of the noise level's definition (tests/noise_spec_numpy.py) on
tests/noise_cases.golden_cases -- image, mask, [quantile_q8] as the case has it (0: the default), and the definition's histogram as its non-zero
(bin, count) pairs and the record [n, m, sigma_q8, 0]; tests/test_noise_cpu.py recomputes them.  Run from the repository root:
    python tests/golden/make_golden_noise.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import noise_cases as cases  # noqa: E402


def main():
    out = {}
    for case in cases.golden_cases():
        r = cases.run_spec(case)
        n = case["name"] + "/"
        bins = np.nonzero(r["hist"])[0]
        out.update({n + "in_image": case["image"], n + "in_mask": case["mask"], n + "quantile": np.array([case["quantile_q8"]], dtype=np.int64),
                    n + "bins": bins.astype(np.int64), n + "counts": r["hist"][bins].astype(np.int64), n + "record": r["record"]})
        print(case["name"], "q", case["quantile_q8"], "record", r["record"].tolist(), "bins", len(bins))
    path = os.path.join(HERE, "golden_noise_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
