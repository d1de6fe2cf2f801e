"""Writes tests/golden/golden_flow_check_v1.npz: the (33, 70) case of tests/flow_check_cases.py and what the flow check's definition
(tests/flow_check_spec_numpy.py) makes of it, at the default parameters and at (a1, a2) = (0.05, 0.02) -- tests/test_flow_check_cpu.py
recomputes them.  Run from the repository root:
    python tests/golden/make_golden_flow_check.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import flow_check_cases as cases  # noqa: E402
import flow_check_spec_numpy as spec  # noqa: E402


def main():
    fwd, bwd, _ = cases.fields(33, 70)
    out = dict(fwd=fwd, bwd=bwd)
    for a1, a2, tag in ((spec.A1_DEFAULT, spec.A2_DEFAULT, "default"), (0.05, 0.02, "tight")):
        r = spec.flow_check(fwd, bwd, a1=a1, a2=a2)
        out.update({tag + "_mask": r["mask"], tag + "_masked": r["masked"], tag + "_resid": r["resid"], tag + "_count": np.int64(r["count"])})
    path = os.path.join(HERE, "golden_flow_check_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
