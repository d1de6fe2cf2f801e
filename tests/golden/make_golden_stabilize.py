"""Writes tests/golden/golden_stabilize_v1.npz: inputs and outputs of the stabiliser's definition (tests/stabilize_spec_numpy.py) at
(5, 3) BGR, (33, 70) BGR and (64, 96) gray with the standard virtual pose, and one 12-frame path with its smoothed path and virtual
poses -- tests/test_stabilize_cpu.py recomputes them.  Run from the repository root:
    python tests/golden/make_golden_stabilize.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import stabilize_cases as cases  # noqa: E402
import stabilize_spec_numpy as spec  # noqa: E402

# (rows, cols, channels, mode, q5_mode, iterations, arguments of cases.inputs)
CASES = [(5, 3, 3, 0, 0, 3, dict(holes=0.4)),
         (33, 70, 3, 0, 1, 2, dict(holes=0.4, block=(8, 20, 10, 14), specials=True)),
         (64, 96, 1, 0, 0, 0, dict(holes=0.5, block=(20, 30, 16, 24), corner=(9, 11)))]


def main():
    out = {}
    for rows, cols, ch, mode, q5, it, kw in CASES:
        K, image, depth = cases.inputs(rows, cols, channels=ch, **kw)
        R, t = oracle_py.pose_table(cases.POSE["v"], cases.POSE["w"], cases.POSE["k"], cases.POSE["gamma"], rows)
        R = np.ascontiguousarray(R).reshape(rows, 9)
        r = spec.stabilize_frame(image, depth, R, t, K, cases.M_STD, cases.m_STD, mode=mode, q5_mode=q5, iterations=it)
        n = "%dx%d/" % (rows, cols)
        out.update({n + "K": np.array(K), n + "modes": np.array([mode, q5, it]), n + "image": image, n + "depth": depth, n + "R": R, n + "t": t,
                    n + "M": cases.M_STD, n + "m": cases.m_STD, n + "out_image": r["image"], n + "out_mask": r["mask"], n + "out_filled": r["filled"],
                    n + "out_disp": r["disp"], n + "out_valid": np.array(r["valid"], dtype=np.int64)})
    p = cases.golden_path()
    As, cs = spec.smooth_path(p["A"], p["c"], p["sigma"], p["radius"])
    M, m = spec.virtual_poses(p["A"], p["c"], As, cs, p["scales"])
    out.update({"path/A": p["A"], "path/c": p["c"], "path/scales": p["scales"], "path/sigma": np.array(p["sigma"]), "path/A_s": As, "path/c_s": cs,
                "path/M": M, "path/m": m})
    path = os.path.join(HERE, "golden_stabilize_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
