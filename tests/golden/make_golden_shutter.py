"""Writes tests/golden/golden_shutter_v1.npz: the outputs of the synthetic shutter's definition (tests/shutter_spec_numpy.py) on every case of
tests/shutter_cases.all_cases -- image, mask, coverage, [unset, partial, full] and the kept sub-instants -- and a digest of the case's inputs;
tests/test_shutter_cpu.py recomputes them.  Run from the repository root:
    python tests/golden/make_golden_shutter.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import shutter_cases as cases  # noqa: E402


def digest(case):
    """a CRC of everything the definition reads"""
    crc = 0
    for k in ("frames", "depths", "Rs", "ts"):
        for a in case[k]:
            crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    for k in ("A", "c", "A_path", "c_path", "scales"):
        crc = zlib.crc32(np.ascontiguousarray(case[k], dtype=np.float64).tobytes(), crc)
    words = list(case["K"]) + list(case["window"]) + [case[k] for k in ("t", "shutter", "samples", "min_samples", "threshold", "occlusion", "search", "tol_q16", "mode",
                                                                         "q5_mode", "iterations")]
    return zlib.crc32(np.asarray(words, dtype=np.float64).tobytes(), crc)


def main():
    out = {}
    for case in cases.all_cases(oracle_py.pose_table):
        r = cases.run_spec(case)
        n = case["name"] + "/"
        out.update({n + "digest": np.array(digest(case), dtype=np.int64), n + "image": r["image"], n + "mask": r["mask"], n + "coverage": r["coverage"],
                    n + "counts": np.array(r["counts"], dtype=np.int64), n + "times": np.array(r["times"], dtype=np.float64)})
        print(case["name"], case["depths"][0].shape, "t", case["t"], "shutter", case["shutter"], "S", case["samples"], "min", case["min_samples"], "kept", len(r["times"]),
              "[unset, partial, full]", r["counts"])
    path = os.path.join(HERE, "golden_shutter_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
