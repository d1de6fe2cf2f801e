"""Writes tests/golden/golden_stabilize_fill_v1.npz: inputs and outputs of the border fill's definition (tests/stabilize_fill_spec_numpy.py)
for frames of tests/stabilize_fill_cases.clip_case -- (33, 70) BGR, frame 1 at radius 2 (offset -2 is outside the clip); (24, 40) gray, frame 3
at radius 1 (offset +1 is the clip's last frame); (5, 3) BGR, frame 2 at radius 2 -- tests/test_stabilize_fill_cpu.py recomputes them.  Run
from the repository root:
    python tests/golden/make_golden_stabilize_fill.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import stabilize_fill_cases as cases  # noqa: E402
import stabilize_fill_spec_numpy as spec  # noqa: E402

# (rows, cols, channels, frame q, radius, mode, q5_mode, iterations)
CASES = [(33, 70, 3, 1, 2, 0, 0, 0), (24, 40, 1, 3, 1, 0, 1, 2), (5, 3, 3, 2, 2, 1, 0, 3)]


def main():
    out = {}
    for rows, cols, ch, q, radius, mode, q5, it in CASES:
        cc = cases.clip_case(oracle_py.pose_table, rows, cols, channels=ch)
        r = spec.stabilize_filled_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], q, cc["M"][q],
                                        cc["m"][q], radius=radius, mode=mode, q5_mode=q5, iterations=it)
        n = "%dx%d/" % (rows, cols)
        out.update({n + "K": np.array(cc["K"]), n + "modes": np.array([q, radius, mode, q5, it]), n + "images": np.stack(cc["images"]),
                    n + "depths": np.stack(cc["depths"]), n + "R": cc["Rs"][0], n + "t": cc["ts"][0], n + "A": cc["A"], n + "c": cc["c"], n + "A_s": cc["As"],
                    n + "c_s": cc["cs"], n + "scales": cc["scales"], n + "M": cc["M"][q], n + "m": cc["m"][q], n + "out_image": r["image"], n + "out_mask": r["mask"],
                    n + "out_source": r["source"], n + "out_counts": np.array(r["counts"], dtype=np.int64)})
    path = os.path.join(HERE, "golden_stabilize_fill_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
