"""Writes tests/golden/golden_erase_v1.npz: the outputs of the mover removal's definition (tests/erase_spec_numpy.py) on every case of
tests/erase_cases.all_cases -- image, mask, matte, the plate's flag and [unset, kept, replaced, feathered, unresolved] -- with a digest of the
case's inputs; tests/test_erase_cpu.py recomputes them.  Run from the repository root:
    python tests/golden/make_golden_erase.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import erase_cases as cases  # noqa: E402
from make_golden_plate import digest as plate_digest  # noqa: E402

PLANES = ("image", "mask", "matte", "moving")


def digest(case):
    """a CRC of everything the definition reads: the plate's digest and the matte's parameters"""
    words = [case[k] for k in ("open", "grow", "feather", "include_undecided")]
    return zlib.crc32(np.asarray(words, dtype=np.float64).tobytes(), plate_digest(case))


def main():
    out = {}
    for case in cases.all_cases(oracle_py.pose_table):
        r = cases.run_spec(case)
        n = case["name"] + "/"
        out.update({n + k: r[k] for k in PLANES})
        out.update({n + "digest": np.array(digest(case), dtype=np.int64), n + "counts": np.array(r["counts"], dtype=np.int64)})
        print(case["name"], case["depths"][0].shape, "q", case["q"], "sources", r["sources"], "(open, grow, feather, undecided)",
              (case["open"], case["grow"], case["feather"], case["include_undecided"]), "[unset, kept, replaced, feathered, unresolved]", r["counts"], "matte",
              sorted(set(np.unique(r["matte"]).tolist())))
    path = os.path.join(HERE, "golden_erase_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
