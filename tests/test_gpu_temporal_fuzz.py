"""GPU: a slice of the temporal stages' randomised campaign (tests/fuzz_temporal.py: the merge, the shutter's, the denoise's and the
super-resolution's chains, the blend's record, the render, the plate's median on planes placed at the minimum alignment the headers admit, and
the five frame calls, interleaved with cases of the existing campaign, bit for bit against their definitions on ONE context per library
build), the cases that ever failed, and the two grid-stride loops of these stages that no other test takes past their first pass:
retime_merge_kernel's and shutter_accumulate_kernel's (1024 blocks of 256 threads of 4 pixels: above 1048576 pixels).

test_campaign_slice takes 4.0 s on the MI355X's host for the first build (its definitions and the probes' among them) and 0.4 s for the second,
which shares them; the two second-trip tests 0.2 s each."""
import numpy as np
import pytest

import retime_cases as rcases
import retime_spec_numpy as retime_spec
import shutter_cases as scases
import shutter_spec_numpy as shutter_spec
import temporal_fuzz_cases as T

pytestmark = pytest.mark.gpu

# 140 cases: the definitions take 1.7 s on one CPU core (tests/test_temporal_fuzz_cpu.py measures and bounds it); the second build shares them
SLICE, SLICE_SEED = 140, 1
ONE_GRID = 1024 * 256 * 4
PAST_ONE_GRID = ((1025, 1028), (1027, 1023))  # 1053700 pixels, every row on a word; 1050621 pixels, npix % 4 = 1: the byte tail runs as well


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_campaign_slice(rsdsfm, arith):
    import fuzz_temporal

    assert fuzz_temporal.main(SLICE, SLICE_SEED, arith, keep_specs=True) == 0


def test_regressions(rsdsfm):
    """every case that ever failed on the GPU (temporal_fuzz_cases.REGRESSIONS), on both library builds"""
    import fuzz_temporal

    for seed in sorted({seed for seed, _ in T.REGRESSIONS}):
        for arith in ("reference", "fused"):
            assert fuzz_temporal.main([n for s, n in T.REGRESSIONS if s == seed], seed, arith, keep_specs=True) == 0, (seed, arith)


def _past(plane):
    return np.asarray(plane).reshape(plane.shape[0] * plane.shape[1], -1)[ONE_GRID:]


def test_merge_past_one_grid(rsdsfm):
    """retime_merge_kernel's loop takes a second trip: gray at (1025, 1028), BGR at (1027, 1023).  Image, mask, source plane and the five
    counters against the definition; behind flat index 1048576 the source plane holds every value the weight admits (0, 1, 2, 3 and 5), and every counter is larger
    than the first trip's pixels alone would make it"""
    import torch

    from test_gpu_retime import _merge, _same

    with rsdsfm.Solver(0) as s:
        for (rows, cols), channels in zip(PAST_ONE_GRID, (1, 3)):
            assert rows * cols > ONE_GRID and ((rows * cols) % 4 == 1) == (cols == 1023)
            ia, ma, ib, mb = rcases.merge_layers(rows, cols, channels)
            want = retime_spec.merge(ia, ma, ib, mb, 32769, 24)
            head = np.bincount(want["source"].reshape(-1)[:ONE_GRID], minlength=6)
            first_trip = [int(head[0]), int(head[1]), int(head[2]), int(head[3]), int(head[4] + head[5])]
            assert set(np.unique(_past(want["source"])).tolist()) == {0, 1, 2, 3, 5} and _past(want["image"]).any()  # (w > 32768: conflicts go to b)
            assert all(w > f for w, f in zip(want["counts"], first_trip))
            got = _merge(torch, s, ia, ma, ib, mb, 32769, 24)
            print((rows, cols), channels, "counts", got["counts"], "of them in the first trip", first_trip)
            _same(got, want, (rows, cols))


def test_shutter_past_one_grid(rsdsfm):
    """shutter_accumulate_kernel's loop takes a second trip in each launch of a three-sample chain (first, mid, last): BGR at (1025, 1028), gray
    at (1027, 1023).  Image, mask, coverage, the three counters and the cells the mid step left against the definition; behind flat index
    1048576 the coverage takes every value 0 .. 3 and every counter is larger than the first trip's pixels alone would make it"""
    import torch

    from test_gpu_shutter import _expose, _same, _spec_cells

    with rsdsfm.Solver(0) as s:
        for (rows, cols), channels in zip(PAST_ONE_GRID, (3, 1)):
            ss = scases.samples(rows, cols, channels, 3)
            want = shutter_spec.expose(ss, 2)
            n = want["coverage"].reshape(-1)[:ONE_GRID]
            first_trip = [int((n < 2).sum()), int((n == 2).sum()), int((n == 3).sum())]
            assert set(np.unique(_past(want["coverage"])).tolist()) == {0, 1, 2, 3} and _past(want["image"]).any()
            assert all(w > f for w, f in zip(want["counts"], first_trip))
            got, cells = _expose(torch, s, ss, 2)
            print((rows, cols), channels, "counts", got["counts"], "of them in the first trip", first_trip)
            _same(got, want, (rows, cols))
            want_cells = _spec_cells(ss, 2)
            assert np.array_equal(cells, want_cells) and _past(want_cells).any()
