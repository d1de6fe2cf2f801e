"""Writes tests/golden/golden_stabilize_visible_v1.npz: the outputs of the occlusion test's definition (tests/stabilize_visible_spec_numpy.py)
on every case of tests/stabilize_visible_cases.all_cases -- image, mask, source and [taken, rejected] -- and a digest of the case's inputs;
tests/test_stabilize_visible_cpu.py recomputes them.  Run from the repository root:
    python tests/golden/make_golden_stabilize_visible.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import stabilize_visible_cases as cases  # noqa: E402


def digest(case):
    """a CRC of everything the definition reads"""
    crc = 0
    for k in ("image", "depth", "R", "t", "M", "m", "mask0", "image0", "source0"):
        crc = zlib.crc32(np.ascontiguousarray(case[k]).tobytes(), crc)
    tail = np.array(list(case["K"]) + list(case["window"]) + [case["tol_q16"], case["mode"], case["q5_mode"], case["iterations"]], dtype=np.float64)
    return zlib.crc32(tail.tobytes(), crc)


def main():
    out = {}
    for case in cases.all_cases(oracle_py.pose_table):
        r = cases.run_spec(case)
        n = case["name"] + "/"
        out.update({n + "digest": np.array(digest(case), dtype=np.int64), n + "image": r["image"], n + "mask": r["mask"], n + "source": r["source"],
                    n + "counts": np.array(r["counts"], dtype=np.int64)})
        print(case["name"], case["depth"].shape, "taken, rejected", r["counts"], "plain", cases.run_spec(case, visible=False)["counts"][0])
    path = os.path.join(HERE, "golden_stabilize_visible_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
