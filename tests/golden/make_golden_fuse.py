"""Writes tests/golden/golden_fuse_v1.npz: the (17, 70) special chain of tests/fuse_cases.py (six pairs) and a (3, 5) chain of three pairs at
tol = 0.01, with what the fusion's definition (tests/fuse_spec_numpy.py) makes of them -- the maps as bit patterns, the fused maps, the flags,
the splat planes and the records (own, filled_prev, filled_next, confirmed, contradicted, left per pair).  tests/test_fuse_cpu.py recomputes
them.  Data only.  Run from the repository root:
    python tests/golden/make_golden_fuse.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import fuse_cases as cases  # noqa: E402
import fuse_spec_numpy as spec  # noqa: E402


def main():
    out = {}
    for tag, ch, kw in (("special", cases.special_chain(17, 70), {}), ("small", cases.chain_case(3, 5, 3, 0.3), dict(tol=0.01))):
        r = spec.fuse(ch["fields"], ch["maps"], ch["vs"], ch["ws"], ch["ks"], ch["records"], ch["K"], ch["gamma"], **kw)
        bits = lambda a: np.ascontiguousarray(np.stack(a), dtype=np.float64).view(np.uint64)
        out[tag + "_maps"], out[tag + "_fused"] = bits(ch["maps"]), bits(r["fused"])
        out[tag + "_flags"], out[tag + "_splat"] = np.stack(r["flags"]), np.stack(r["splat"])
        out[tag + "_records"] = np.array([[x[k] for k in spec.RECORD_FIELDS] for x in r["records"]], dtype=np.int64)
    path = os.path.join(HERE, "golden_fuse_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
