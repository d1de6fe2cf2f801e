#!/usr/bin/env python3
"""Records golden_flow_spec_v1.npz: two cases of tests/test_gpu_flow.py::test_bit_identical_to_spec (the 37x53 pair with 3 channels at
the default parameters, the 60x96 pair with 1 channel at the non-default ones) with the float32 spec's field, so that a change of
tests/flow_spec_numpy.py that moves a bit of the float32 path is seen on the CPU (tests/test_flow_cpu.py).  The field is float32
widened to float64, so it is stored as float32 without loss.  Run once, from the commit whose spec is to be pinned:
    python tests/golden/make_golden_flow.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import flow_spec_numpy as S  # noqa: E402
import rsdsfm  # noqa: E402

NONDEFAULT = dict(fixed_point_iterations=2, sor_iterations=7, downscale=0.8)


def pair(rows, cols, seed):
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, 0.8, _model_only=True)
    s = 2.0 / np.abs(f0).max()
    a, b, _, _ = rsdsfm.synth.render_pair(rows, cols, K, v * s, w * s, k, 0.8, seed=seed)
    return a, b


if __name__ == "__main__":
    out = {}
    a, b = pair(37, 53, 37 + 53)
    f = S.deep_flow(a, b)
    assert np.array_equal(f, f.astype(np.float32).astype(np.float64))
    out.update(a_37x53=a, b_37x53=b, flow_37x53=f.astype(np.float32))
    a, b = pair(60, 96, 60 + 96)
    a, b = a[..., 1].copy(), b[..., 1].copy()
    f = S.deep_flow(a, b, **NONDEFAULT)
    assert np.array_equal(f, f.astype(np.float32).astype(np.float64))
    out.update(a_60x96=a, b_60x96=b, flow_60x96=f.astype(np.float32))
    path = os.path.join(HERE, "golden_flow_spec_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
