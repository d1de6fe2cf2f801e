"""Writes the temporal noise curve's two fixtures.
tests/golden/golden_noise_temporal_v1.npz: the inputs and the outputs of the definition (tests/noise_temporal_spec_numpy.py) on
tests/noise_temporal_cases.golden_cases -- reference, layer and their masks, the pair histogram as its non-zero (key, count) pairs -- and one
frame: the noisy shift clip's middle frame with its four registered neighbours and records, the summed histogram and the curve.
tests/golden/noise_temporal_calls_v1.json.gz: what every function of rsdsfm_noise_temporal.py hands the library on tests/binding_recorder.py's
stand-in (tests/noise_temporal_binding_cases.py's table of calls).  tests/test_noise_temporal_cpu.py recomputes both.  Run from the repository
root:
    python tests/golden/make_golden_noise_temporal.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import binding_recorder as rec  # noqa: E402
import noise_temporal_binding_cases as bcases  # noqa: E402
import noise_temporal_cases as cases  # noqa: E402


def sparse(hist):
    """the non-zero words of a histogram -> (n, 2) int64 [key, count]"""
    flat = np.asarray(hist).reshape(-1).astype(np.int64)
    keys = np.flatnonzero(flat)
    return np.stack([keys, flat[keys]], axis=1)


def main():
    out = {}
    for case in cases.golden_cases():
        n = case["name"] + "/"
        hist = cases.run_spec(case)
        out.update({n + "ref": case["ref"], n + "rmask": case["rmask"], n + "layer": case["layer"], n + "lmask": case["lmask"], n + "hist": sparse(hist)})
        print(case["name"], int(hist.sum()), "samples")
    m = cases.shift_measure(3, 6, 0)
    ref, rmask, _ = m["run"]["ref"]
    out.update({"frame/ref": ref, "frame/rmask": rmask, "frame/records": m["run"]["records"], "frame/hist": sparse(m["temporal"]["hist"]), "frame/curve": m["temporal"]["curve"]})
    for j, (image, mask) in enumerate(m["run"]["layers"]):
        out.update({"frame/layer%d" % j: image, "frame/lmask%d" % j: mask})
    path = os.path.join(HERE, "golden_noise_temporal_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")

    import rsdsfm
    import rsdsfm_noise_temporal as nt

    calls = {name: rec.run_case(rsdsfm, lambda e, fn=fn: fn(e, nt)) for name, fn in bcases.CASES}
    path = os.path.join(HERE, "noise_temporal_calls_v1.json.gz")
    rec.write_gz(path, {"cases": calls})
    print(path, os.path.getsize(path), "bytes", len(calls), "cases")


if __name__ == "__main__":
    main()
