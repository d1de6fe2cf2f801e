"""Writes tests/golden/golden_link_v1.npz: the (17, 70) special case of tests/link_cases.py and what the link's definition
(tests/link_spec_numpy.py) makes of it -- the ratio plane and the record at the default parameters and at tol = 0.01 -- and a chain of seven
pairs with one broken link -- tests/test_link_cpu.py recomputes them -- and the four 48 x 64 frames synth.render_sequence gave for a constant
motion before it had its `speeds` argument (seq_frames: written with speeds=None, which must stay that code path).  Run from the repository root:
    python tests/golden/make_golden_link.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import link_cases as cases  # noqa: E402
import link_spec_numpy as spec  # noqa: E402


def chain_inputs():
    r = np.random.default_rng(20261018)
    vs, ws = r.normal(size=(7, 3)) * 0.05, r.normal(size=(7, 3)) * 0.02
    ratios, valids = r.uniform(0.5, 2.0, size=6), np.array([1, 1, 1, 0, 1, 1], dtype=np.uint8)
    return vs, ws, ratios, valids


def main():
    d, _ = cases.special_case(17, 70)
    out = dict(F=d["F"], Zp=d["Zp"], Zn=d["Zn"], v=d["v"], w=d["w"], k=np.float64(d["k"]), K=np.array(d["K"]), gamma=np.float64(d["gamma"]))
    for tol, tag in ((spec.TOL_DEFAULT, "default"), (0.01, "tight")):
        r = spec.link(d["F"], d["Zp"], d["v"], d["w"], d["k"], d["Zn"], d["K"], d["gamma"], tol=tol)
        out.update({tag + "_plane": r["plane"], tag + "_n": np.int64(r["n"]), tag + "_ratio": np.float64(r["ratio"]), tag + "_agree": np.int64(r["agree"])})
    vs, ws, ratios, valids = chain_inputs()
    ch = spec.chain(ratios, valids, vs, ws, cases.GAMMA)
    out.update(chain_v=vs, chain_w=ws, chain_ratios=ratios, chain_valids=valids, chain_scales=ch["scales"], chain_A=ch["A"], chain_c=ch["c"],
               chain_broken=ch["broken"])
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import rsdsfm

    out["seq_frames"] = rsdsfm.synth.render_sequence(4, 48, 64, (48.0, 48.0, 32.0, 24.0), *rsdsfm.synth.default_motion(), gamma=0.8, seed=11)[0]
    path = os.path.join(HERE, "golden_link_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
