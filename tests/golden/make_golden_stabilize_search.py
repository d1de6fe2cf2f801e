"""Writes tests/golden/golden_stabilize_search_v1.npz: the outputs of the visible pre-image search's definition
(tests/stabilize_search_spec_numpy.py) on every case of tests/stabilize_search_cases.all_cases -- image, mask, source and [taken, rejected,
recovered] -- and a digest of the case's inputs; tests/test_stabilize_search_cpu.py recomputes them.  Run from the repository root:
    python tests/golden/make_golden_stabilize_search.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import stabilize_search_cases as cases  # noqa: E402
from make_golden_stabilize_visible import digest  # noqa: E402,F401  (the same CRC of everything the definition reads)


def main():
    out = {}
    for case in cases.all_cases(oracle_py.pose_table):
        r = cases.run_spec(case)
        n = case["name"] + "/"
        out.update({n + "digest": np.array(digest(case), dtype=np.int64), n + "image": r["image"], n + "mask": r["mask"], n + "source": r["source"],
                    n + "counts": np.array(r["counts"], dtype=np.int64)})
        print(case["name"], case["depth"].shape, "taken, rejected, recovered", r["counts"], "visible", cases.run_visible(case)["counts"])
    path = os.path.join(HERE, "golden_stabilize_search_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
