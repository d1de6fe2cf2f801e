"""Writes the sharpen stage's two fixtures.
tests/golden/golden_sharpen_v1.npz: the inputs, the parameters and the outputs of the definition (tests/sharpen_spec_numpy.py) on
tests/sharpen_cases.golden_cases -- image, mask, [amount_q4, coring_q4, overshoot, strength], the output image and the four counters -- and one
case through a hand-made rising curve's strength table.
tests/golden/sharpen_calls_v1.json.gz: what every function of rsdsfm_sharpen.py hands the library on tests/binding_recorder.py's stand-in
(tests/sharpen_binding_cases.py's table of calls).  tests/test_sharpen_cpu.py recomputes both.  Run from the repository root:
    python tests/golden/make_golden_sharpen.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import binding_recorder as rec  # noqa: E402
import sharpen_binding_cases as bcases  # noqa: E402
import sharpen_cases as cases  # noqa: E402
import sharpen_spec_numpy as spec  # noqa: E402


def main():
    out = {}
    for case in cases.golden_cases():
        r = cases.run_spec(case)
        n = case["name"] + "/"
        out.update({n + "in_image": case["image"], n + "in_mask": case["mask"],
                    n + "params": np.array([case["amount_q4"], case["coring_q4"], case["overshoot"], case["strength"]], dtype=np.int64), n + "image": r["image"],
                    n + "counts": np.array(r["counts"], dtype=np.int64)})
        print(case["name"], out[n + "params"].tolist(), r["counts"])
    image, mask, lut = cases.golden_curve_case()
    r = spec.sharpen(image, mask, lut=lut)
    out.update({"curve/in_image": image, "curve/in_mask": mask, "curve/lut": lut, "curve/image": r["image"], "curve/counts": np.array(r["counts"], dtype=np.int64)})
    path = os.path.join(HERE, "golden_sharpen_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")

    import rsdsfm
    import rsdsfm_sharpen as sh

    calls = {name: rec.run_case(rsdsfm, lambda e, fn=fn: fn(e, sh)) for name, fn in bcases.CASES}
    path = os.path.join(HERE, "sharpen_calls_v1.json.gz")
    rec.write_gz(path, {"cases": calls})
    print(path, os.path.getsize(path), "bytes", len(calls), "cases")


if __name__ == "__main__":
    main()
