#!/usr/bin/env python3
"""Randomised GPU-vs-spec campaign of the DeepFlow front end (not collected by pytest: run  python tests/fuzz_flow.py [cases] [seed]
on a GPU box; tests/test_gpu_flow_edges.py runs a slice of it).

Case n of campaign `seed` is flow_cases.random_case(n, seed): sides in [2, 200] biased to {2, 3, 63..66, 95..98}, 1 or 3 channels, a
content kind of tests/flow_cases.py, parameters over the ranges include/rsdsfm_flow.h documents.  Even cases go through
rsdsfm_deep_flow, odd ones through a 3-frame rsdsfm_deep_flow_seq (batch size drawn from 1 / 2 / default); every field is compared
with tests/flow_spec_numpy.py bit for bit.  A spec field that is not finite is a failure (of the spec), never a skip.  Prints one
line per failing case with everything needed to rebuild it and a summary; returns 1 if anything failed.

Environment: FUZZ_ONLY=3,17 re-runs selected case numbers of a campaign (same cases / seed arguments)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import flow_cases as FC  # noqa: E402
import flow_spec_numpy as S  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_case(solver, case, through_seq, batch=0):
    """-> list of failure strings (empty when the case is clean)"""
    nframes = 3 if through_seq else 2
    fr = FC.frames(case, nframes)
    if through_seq:
        solver.set_flow_batch(batch)
        got = solver.deep_flow_seq(fr, case.params)
        solver.set_flow_batch(0)
    else:
        got = solver.deep_flow(fr[0], fr[1], case.params)[None]
    fails = []
    for p in range(nframes - 1):
        want = S.deep_flow(fr[p], fr[p + 1], **case.params)
        if not np.isfinite(want).all():
            fails.append("pair %d: the SPEC is not finite (%d of %d values)" % (p, int((~np.isfinite(want)).sum()), want.size))
        elif got[p].shape != want.shape:
            fails.append("pair %d: shape %s, expected %s" % (p, got[p].shape, want.shape))
        elif not np.array_equal(_bits(got[p]), _bits(want)):
            diff = _bits(got[p]) != _bits(want)
            with np.errstate(invalid="ignore"):
                fails.append("pair %d: %d of %d values differ, max |diff| %.3g, GPU finite: %s" % (p, int(diff.sum()), diff.size, np.nanmax(np.abs(got[p] - want)),
                                                                                                 bool(np.isfinite(got[p]).all())))
    return fails


def main(cases=None, seed=None):
    import rsdsfm

    cases = int(sys.argv[1]) if cases is None and len(sys.argv) > 1 else (cases or 60)
    seed = int(sys.argv[2]) if seed is None and len(sys.argv) > 2 else (seed or 1)
    only = [int(x) for x in os.environ.get("FUZZ_ONLY", "").split(",") if x]
    bad = 0
    with rsdsfm.Solver(0) as s:
        for n in only or range(cases):
            case = FC.random_case(n, seed)
            through_seq = bool(n % 2)
            batch = (1, 2, 0)[(n // 2) % 3]
            try:
                fails = check_case(s, case, through_seq, batch)
            except Exception as e:  # a rejected call is a failure too: every drawn parameter set is a documented one
                fails = ["%s: %s" % (type(e).__name__, e)]
            if fails:
                bad += 1
                print("FAIL seed %d case %d (%s, batch %d): %dx%d x%d kind %s frame seed %d params %r" % (
                    seed, n, "deep_flow_seq" if through_seq else "deep_flow", batch, case.rows, case.cols, case.channels, case.kind, case.seed, case.params))
                for f in fails:
                    print("    " + f)
    print("fuzz_flow: %d cases (seed %d), %d failed" % (len(only) if only else cases, seed, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
