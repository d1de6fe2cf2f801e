"""Writes the noise curve's two fixtures.
tests/golden/golden_noise_curve_v1.npz: the inputs, the quantile and the outputs of the definition (tests/noise_curve_spec_numpy.py) on
tests/noise_curve_cases.golden_cases -- image, mask, [quantile_q8], the banded histogram as its non-zero (key, count) pairs (key = band << 10 |
bin), the curve (9, 4) and the strength table at the cases' min_samples and band_min_samples -- and the tables of the hand-made curves.
tests/golden/noise_curve_calls_v1.json.gz: what every function of rsdsfm_noise_curve.py hands the library on tests/binding_recorder.py's
stand-in (tests/noise_curve_cases.py's table of calls).  tests/test_noise_curve_cpu.py recomputes both.  Run from the repository root:
    python tests/golden/make_golden_noise_curve.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import binding_recorder as rec  # noqa: E402
import noise_curve_binding_cases as bcases  # noqa: E402
import noise_curve_cases as cases  # noqa: E402
import noise_curve_spec_numpy as spec  # noqa: E402


def main():
    out = {}
    for case in cases.golden_cases():
        r = cases.run_spec(case)
        n = case["name"] + "/"
        flat = r["hist"].reshape(-1)
        keys = np.nonzero(flat)[0]
        out.update({n + "in_image": case["image"], n + "in_mask": case["mask"], n + "quantile": np.array([case["quantile_q8"]], dtype=np.int64),
                    n + "keys": keys.astype(np.int64), n + "counts": flat[keys].astype(np.int64), n + "curve": r["curve"],
                    n + "lut": spec.strengths(r["curve"], 0, 12, cases.MIN_SAMPLES, cases.BAND_MIN_SAMPLES)})
        print(case["name"], "q", case["quantile_q8"], "n", r["curve"][:, 0].tolist(), "m", r["curve"][:, 1].tolist())
    for k, (curve, fallback, scale, ms, bms) in enumerate(cases.CURVES):
        out["curves/%d" % k] = curve
        out["curves/%d/lut" % k] = spec.strengths(curve, scale, fallback or 12, ms, bms)
    path = os.path.join(HERE, "golden_noise_curve_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")

    import rsdsfm
    import rsdsfm_noise_curve as nc

    calls = {name: rec.run_case(rsdsfm, lambda e, fn=fn: fn(e, nc)) for name, fn in bcases.CASES}
    path = os.path.join(HERE, "noise_curve_calls_v1.json.gz")
    rec.write_gz(path, {"cases": calls})
    print(path, os.path.getsize(path), "bytes", len(calls), "cases")


if __name__ == "__main__":
    main()
