"""Writes tests/golden/golden_deblur_v1.npz: the outputs of the sharpness transfer's definition (tests/deblur_spec_numpy.py) on every case of
tests/deblur_cases.all_cases -- image, mask, weight plane, [unset, own only, transferred], the overlap records, the sharpness records and the
taus -- and a digest of the case's inputs; tests/test_deblur_cpu.py recomputes them.  Run from the repository root:
    python tests/golden/make_golden_deblur.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import deblur_cases as cases  # noqa: E402


def digest(case):
    """a CRC of everything the definition reads"""
    crc = 0
    for k in ("frames", "depths", "Rs", "ts"):
        for a in case[k]:
            crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    for k in ("A", "c", "A_path", "c_path", "scales"):
        crc = zlib.crc32(np.ascontiguousarray(case[k], dtype=np.float64).tobytes(), crc)
    words = list(case["K"]) + list(case["window"]) + [case[k] for k in ("q", "radius", "strength", "margin", "min_pairs", "gate_mode", "min_overlap", "gain_mode", "occlusion",
                                                                         "search", "tol_q16", "mode", "q5_mode", "iterations")]
    return zlib.crc32(np.asarray(words, dtype=np.float64).tobytes(), crc)


def main():
    out = {}
    for case in cases.all_cases(oracle_py.pose_table):
        r = cases.run_spec(case)
        n = case["name"] + "/"
        out.update({n + "digest": np.array(digest(case), dtype=np.int64), n + "image": r["image"], n + "mask": r["mask"], n + "weight": r["weight"],
                    n + "counts": np.array(r["counts"], dtype=np.int64), n + "records": r["records"], n + "sharps": r["sharps"], n + "taus": np.array(r["taus"], dtype=np.int32)})
        print(case["name"], case["depths"][0].shape, "q", case["q"], "sources", r["sources"], "h", case["strength"], "taus", r["taus"], "[unset, own only, transferred]",
              r["counts"], "largest weight", int(r["weight"].max()))
    path = os.path.join(HERE, "golden_deblur_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
