"""Writes tests/golden/golden_retime_v1.npz: the outputs of the retimer's definition (tests/retime_spec_numpy.py) on every case of
tests/retime_cases.all_cases -- image, mask, source and [none, a only, b only, dissolved, conflict] -- and a digest of the case's inputs;
tests/test_retime_cpu.py recomputes them.  Run from the repository root:
    python tests/golden/make_golden_retime.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import retime_cases as cases  # noqa: E402


def digest(case):
    """a CRC of everything the definition reads"""
    crc = 0
    for k in ("images", "depths", "Rs", "ts"):
        for a in case[k]:
            crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    for k in ("M", "m"):
        crc = zlib.crc32(np.ascontiguousarray(case[k], dtype=np.float64).tobytes(), crc)
    words = list(case["K"]) + list(case["window"]) + [case[k] for k in ("weight", "threshold", "occlusion", "search", "tol_q16", "mode", "q5_mode", "iterations")]
    return zlib.crc32(np.asarray(words, dtype=np.float64).tobytes(), crc)


def main():
    out = {}
    for case in cases.all_cases(oracle_py.pose_table):
        r = cases.run_spec(case)
        n = case["name"] + "/"
        out.update({n + "digest": np.array(digest(case), dtype=np.int64), n + "image": r["image"], n + "mask": r["mask"], n + "source": r["source"],
                    n + "counts": np.array(r["counts"], dtype=np.int64)})
        print(case["name"], case["depths"][0].shape, "sources", len(case["images"]), "weight", case["weight"], "threshold", case["threshold"],
              "[none, a only, b only, dissolved, conflict]", r["counts"])
    path = os.path.join(HERE, "golden_retime_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
