"""Writes tests/golden/golden_plate_medoid_v1.npz: the outputs of the colour-consistent plate's definition (tests/plate_medoid_spec_numpy.py) on
every case of tests/plate_cases.all_cases -- plate, mask, votes, flag plane, [unset, static, moving, undecided] and the records -- with
make_golden_plate's digest of the case's inputs, and on make_golden_plate's small cases of the estimator alone; tests/test_plate_medoid_cpu.py
recomputes them.  Run from the repository root:
    python tests/golden/make_golden_plate_medoid.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import plate_cases as cases  # noqa: E402
import plate_medoid_spec_numpy as spec  # noqa: E402
from make_golden_plate import digest, median_cases  # noqa: E402


def main():
    out = {}
    for case in cases.all_cases(oracle_py.pose_table):
        r = spec.run_spec(case)
        n = case["name"] + "/"
        out.update({n + "digest": np.array(digest(case), dtype=np.int64), n + "image": r["image"], n + "mask": r["mask"], n + "votes": r["votes"], n + "moving": r["moving"],
                    n + "counts": np.array(r["counts"], dtype=np.int64), n + "records": r["records"]})
        print(case["name"], case["depths"][0].shape, "q", case["q"], "sources", r["sources"], "tau", case["threshold"], "min_votes", case["min_votes"],
              "[unset, static, moving, undecided]", r["counts"], "differs from the median in", int((r["image"] != cases.run_spec(case)["image"]).sum()), "bytes")
    for name, case in median_cases().items():
        r = spec.spec_of(case)
        out.update({name + "/image": r["image"], name + "/mask": r["mask"], name + "/votes": r["votes"], name + "/moving": r["moving"],
                    name + "/counts": np.array(r["counts"], dtype=np.int64)})
        print(name, "[unset, static, moving, undecided]", r["counts"])
    path = os.path.join(HERE, "golden_plate_medoid_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
