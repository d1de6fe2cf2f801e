"""Writes tests/golden/golden_plate_v1.npz: the outputs of the clean plate's definition (tests/plate_spec_numpy.py) on every case of
tests/plate_cases.all_cases -- plate, mask, votes, flag plane, [unset, static, moving, undecided] and the records -- with a digest of the case's
inputs, and on a few small cases of the median alone; tests/test_plate_cpu.py recomputes them.  Run from the repository root:
    python tests/golden/make_golden_plate.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import plate_cases as cases  # noqa: E402


def digest(case):
    """a CRC of everything the definition reads"""
    crc = 0
    for k in ("frames", "depths", "Rs", "ts"):
        for a in case[k]:
            crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    for k in ("A", "c", "A_path", "c_path", "scales"):
        crc = zlib.crc32(np.ascontiguousarray(case[k], dtype=np.float64).tobytes(), crc)
    words = list(case["K"]) + list(case["window"]) + [case[k] for k in ("q", "radius", "threshold", "min_votes", "min_overlap", "gain_mode", "occlusion", "search", "tol_q16",
                                                                         "mode", "q5_mode", "iterations")]
    return zlib.crc32(np.asarray(words, dtype=np.float64).tobytes(), crc)


def median_cases():
    """name -> the median alone on small inputs: an odd and an even number of candidates, the most layers, gray and BGR, every record"""
    out = {}
    for shape, ch, L in (((5, 5), 3, 3), ((17, 65), 1, 7), ((3, 7), 3, 14), ((16, 64), 1, 0), ((15, 63), 3, 4)):
        ref, rmask, ls = cases.median_inputs(shape, ch, L)
        threshold, min_votes = cases.median_parameters(shape, L)
        out["median-%dx%d-%d-%d" % (shape + (ch, L))] = dict(ref=ref, rmask=rmask, layers=ls, records=cases.layer_records(ch, L) if L else None, min_overlap=0, gain_mode=0,
                                                             threshold=threshold, min_votes=min_votes)
    return out


def main():
    out = {}
    for case in cases.all_cases(oracle_py.pose_table):
        r = cases.run_spec(case)
        n = case["name"] + "/"
        out.update({n + "digest": np.array(digest(case), dtype=np.int64), n + "image": r["image"], n + "mask": r["mask"], n + "votes": r["votes"], n + "moving": r["moving"],
                    n + "counts": np.array(r["counts"], dtype=np.int64), n + "records": r["records"]})
        print(case["name"], case["depths"][0].shape, "q", case["q"], "sources", r["sources"], "tau", case["threshold"], "min_votes", case["min_votes"],
              "[unset, static, moving, undecided]", r["counts"], "votes", sorted(set(np.unique(r["votes"]).tolist())))
    for name, case in median_cases().items():
        r = cases.spec_of(case)
        out.update({name + "/image": r["image"], name + "/mask": r["mask"], name + "/votes": r["votes"], name + "/moving": r["moving"],
                    name + "/counts": np.array(r["counts"], dtype=np.int64)})
        print(name, "[unset, static, moving, undecided]", r["counts"])
    path = os.path.join(HERE, "golden_plate_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
