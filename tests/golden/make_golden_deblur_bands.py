"""Writes tests/golden/golden_deblur_bands_v1.npz: the outputs of the definition of the sharpness transfer per scanline band
(tests/deblur_bands_spec_numpy.py) on every case of tests/deblur_bands_cases.accumulate_cases and frame_cases -- image, mask, weight plane,
[unset, own only, transferred], the band records and the band taus -- and a digest of the case's inputs; tests/test_deblur_bands_cpu.py
recomputes them.  Run from the repository root:
    python tests/golden/make_golden_deblur_bands.py
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import deblur_bands_cases as bcases  # noqa: E402


def digest(case):
    """a CRC of everything the definition reads"""
    crc = 0
    if "ref" in case:
        arrays = [case["ref"], case["rmask"]] + [a for pair in case["layers"] for a in pair] + [np.zeros(8, dtype=np.uint64) if r is None else r for r in case["records"]]
        words = [case["band_rows"]] + [case["kw"][k] for k in sorted(case["kw"])]
    else:
        arrays = [a for k in ("frames", "depths", "Rs", "ts") for a in case[k]] + [np.asarray(case[k], dtype=np.float64) for k in ("A", "c", "A_path", "c_path", "scales")]
        words = list(case["K"]) + list(case["window"]) + [case[k] for k in ("q", "radius", "strength", "margin", "min_pairs", "gate_mode", "min_overlap", "gain_mode", "band_rows")]
    for a in arrays:
        crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    return zlib.crc32(np.asarray(words, dtype=np.float64).tobytes(), crc)


def results():
    """-> [(case, the definition's dict)]"""
    return [(c, bcases.run_accumulate(c)) for c in bcases.accumulate_cases()] + [(c, bcases.run_frame(c)) for c in bcases.frame_cases()]


def main():
    out = {}
    for case, r in results():
        n = case["name"] + "/"
        out.update({n + "digest": np.array(digest(case), dtype=np.int64), n + "image": r["image"], n + "mask": r["mask"], n + "weight": r["weight"],
                    n + "counts": np.array(r["counts"], dtype=np.int64), n + "band_records": r["band_records"], n + "band_taus": np.array(r["band_taus"], dtype=np.int32)})
        print(case["name"], "band taus", r["band_taus"], "[unset, own only, transferred]", r["counts"], "largest weight", int(r["weight"].max()))
    path = os.path.join(HERE, "golden_deblur_bands_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
