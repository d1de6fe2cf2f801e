"""GPU: the DeepFlow front end at the edges its ABI admits -- hostile content, every documented parameter range, the frame sizes that
sit on the borders of the SOR tiling (one region up to 64 x 64; above it regions of interior 48 with a halo of 8 and 4 iterations per
launch), full video sizes with hundreds of regions per launch, clips through the batched path, and a random campaign.  Every field is
the numpy spec's (tests/flow_spec_numpy.py) bit for bit, signed zeros included.  The inputs are the seeded tables of
tests/flow_cases.py; tests/test_flow_cpu.py shows on the CPU that every one of them is finite in the spec.

Before the pyramid stopped at a side of 2, the three `min0_down*` cases were NaN in every value, in the spec and (same expressions)
in the kernels."""
import numpy as np
import pytest

import flow_cases as FC

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.isfinite(want).all()
    diff = _bits(got) != _bits(want)
    with np.errstate(invalid="ignore"):
        assert not diff.any(), "%d of %d values differ, max |diff| %.3g, first at %s" % (diff.sum(), diff.size, np.nanmax(np.abs(got - want)),
                                                                                      tuple(np.argwhere(diff)[0]))


@pytest.fixture(scope="module")
def solver(rsdsfm):
    with rsdsfm.Solver(0) as s:
        yield s


@pytest.mark.parametrize("case", FC.CONTENT, ids=lambda c: c.id)
def test_content(solver, case):
    a, b = FC.pair(case)
    got = solver.deep_flow(a, b, case.params or None)
    _same(got, FC.spec(case))
    if case.cls == "zero":
        assert not _bits(got).any()  # a constant pair: every bit zero, no negative zero


@pytest.mark.parametrize("case", FC.PARAMS, ids=lambda c: c.id)
def test_parameter_ranges(solver, case):
    a, b = FC.pair(case)
    got = solver.deep_flow(a, b, case.params)
    _same(got, FC.spec(case))
    if case.cls == "zero":
        assert not _bits(got).any()  # no data term: the field is exactly zero
    else:
        assert np.abs(got).max() > 0.1


@pytest.mark.parametrize("case", FC.GEOMETRY + FC.FULL, ids=lambda c: c.id)
def test_geometry(solver, case):
    a, b = FC.pair(case)
    got = solver.deep_flow(a, b, case.params)
    _same(got, FC.spec(case))
    assert np.abs(got).max() > 1e-3


@pytest.mark.parametrize("case", FC.CLIPS, ids=lambda c: c.id)
def test_clips(solver, case):
    """4 frames through rsdsfm_deep_flow_seq in batches of 3 pairs and of 2 + 1: each pair against the spec"""
    fr = FC.frames(case, 4)
    try:
        for batch in (3, 2):
            solver.set_flow_batch(batch)
            got = solver.deep_flow_seq(fr, case.params or None)
            assert got.shape == (3,) + FC.spec(case).shape
            for p in range(3):
                _same(got[p], FC.spec(case, p))
    finally:
        solver.set_flow_batch(0)


def test_clip_of_identical_frames_is_all_zero(solver):
    fr = FC.frames(FC.STILL, 4)
    assert np.array_equal(fr[0], fr[3]) and fr.std() > 10.0
    got = solver.deep_flow_seq(fr)
    assert got.shape == (3, 70, 100, 2) and not _bits(got).any()
    assert not _bits(FC.spec(FC.STILL)).any()


def test_fuzz_campaign_slice():
    """60 cases of tests/fuzz_flow.py (random sizes around the tiling's edges, contents, channels and parameters; alternately one
    pair and a 3-frame clip) against the spec bit for bit.  `python tests/fuzz_flow.py 500 <seed>` is the long form."""
    import fuzz_flow

    assert fuzz_flow.main(60, 1) == 0
