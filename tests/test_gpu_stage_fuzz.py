"""GPU: a slice of the stages' randomised campaign (tests/fuzz_stages.py: flow check, link, fusion, dense rectifier, stabiliser, fill, crop,
seam blend and inpainting, drawn at random sizes and parameters, bit for bit against their definitions on ONE context per library build), the
cases that ever failed, and the two grid-stride loops that no other test takes past their first pass: stabilize_count_kernel's (1024 blocks of
256 words: above 1048576 pixels) and crop_search_kernel's (8192 blocks of 256 anchors: above 2097152)."""
import numpy as np
import pytest

import stabilize_cases as stab_cases
import stabilize_crop_cases as crop_cases
import stage_fuzz_cases as G

pytestmark = pytest.mark.gpu

# 120 cases: the definitions take 1.9 s on one CPU core (tests/test_stage_fuzz_cpu.py measures and bounds it) and the first build's test 3.1 s on
# the MI355X's host; the second build shares them (0.3 s)
SLICE, SLICE_SEED = 120, 1


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_campaign_slice(rsdsfm, arith):
    import fuzz_stages

    assert fuzz_stages.main(SLICE, SLICE_SEED, arith, keep_specs=True) == 0


def test_regressions(rsdsfm):
    """every case that ever failed on the GPU (stage_fuzz_cases.REGRESSIONS), on both library builds"""
    import fuzz_stages

    for seed in sorted({seed for seed, _ in G.REGRESSIONS}):
        for arith in ("reference", "fused"):
            assert fuzz_stages.main([n for s, n in G.REGRESSIONS if s == seed], seed, arith, keep_specs=True) == 0, (seed, arith)


def test_count_past_one_grid(oracle, rsdsfm):
    """(1025, 1028): 1053700 pixels, every row on a word; (1027, 1023): 1050621 pixels, npix % 4 = 1, so the byte tail runs as well -- the
    smallest frames at which stabilize_count_kernel's loop takes a second trip.  The count is the downloaded mask's own sum, and pixels past
    the first trip's 1048576 contribute to it."""
    import torch

    dev = torch.device("cuda", 0)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with rsdsfm.Solver(0) as s:
        for rows, cols in ((1025, 1028), (1027, 1023)):
            assert rows * cols > 1024 * 256 * 4 and ((rows * cols) % 4 == 1) == (cols == 1023)
            K, image, depth = crop_cases.inputs(rows, cols, channels=1, holes=0.4)
            R, t = oracle.pose_table(crop_cases.POSE["v"], crop_cases.POSE["w"], crop_cases.POSE["k"], crop_cases.POSE["gamma"], rows)
            d_img, d_dm, d_R, d_t = tt(image), tt(depth.T), tt(np.ascontiguousarray(R).reshape(rows, 9)), tt(t)
            out, d_mask = torch.full_like(d_img, 77), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
            valid = torch.full((3,), -7, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            s.stabilize_frame_dev(d_img.data_ptr(), 1, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K, rows, cols, stab_cases.M_STD, stab_cases.m_STD, out.data_ptr(),
                                  d_mask.data_ptr(), d_valid=valid[1:].data_ptr())
            s.synchronize()
            mask, v = d_mask.cpu().numpy(), valid.cpu().numpy().tolist()
            print((rows, cols), "valid", v[1], "of", rows * cols, "past the first trip", int(mask.reshape(-1)[1048576:].sum()))
            assert set(np.unique(mask).tolist()) == {0, 1}  # zeros and ones, nothing else
            assert mask.reshape(-1)[1048576:].sum() > 0     # the second trip contributes
            assert v[0] == -7 and v[2] == -7 and v[1] == int(mask.sum(dtype=np.int64))


def test_window_search_past_one_grid(rsdsfm):
    """(1500, 1500), 2250000 anchors, all empty but a set square inside rows 1420 .. 1499: with max_empty = 0 and margin = 0 every admissible
    anchor has a linear index above 2097152, so the window comes from crop_search_kernel's second trip; with a larger square in the first
    rows as well the winner comes from the first trip and must survive the second.  The answers are the planted squares by construction (the
    definition takes 4 s per search at this size here; tests/test_stage_fuzz_cpu.py checks it on the same layout at (150, 150))."""
    import torch

    from test_gpu_stabilize_crop import _window

    low, top = G.planted_window(1500), G.planted_window(1500, second=True)
    assert low == (1430, 700, 60, 60) and 1420 <= low[0] and low[0] + low[2] <= 1500 and low[0] * 1500 > 8192 * 256 and top == (10, 300, 70, 70)
    with rsdsfm.Solver(0) as s:
        assert _window(torch, s, [G.planted_mask(1500, [low])], 0, 0) == low
        assert _window(torch, s, [G.planted_mask(1500, [low, top])], 0, 0) == top
        assert _window(torch, s, [G.planted_mask(1500, [low])], 0, 0) == low  # (the key of the call before is gone)
