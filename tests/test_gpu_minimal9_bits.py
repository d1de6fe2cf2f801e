"""The minimal solver's three forms return the same bits: one hypothesis per WAVE with the rotations through the in-range function
cores (what a RANSAC runs), the same with the standard functions, and one hypothesis per LANE (jacobi_svd9_nullvec, the in-repo
reference of the 9x9 Jacobi SVD).  All eight outputs per hypothesis (w, v, k, status) are compared bit for bit, NaNs as equal, and the
two wave forms must agree on the SVD's sweep and rotation counts (rsdsfm_minimal9_probe_dev).

Inputs: random 9-point sets of 96x128 synthetic frames (DeepFlow-like and noise-free), with and without the k estimation, and degenerate
sets -- a repeated point, all-zero flow, nine collinear points -- in front of them.  Counts 1, 50 and 512 (512 = 2 x the CUs: the largest
launch of the wave-per-hypothesis kernel)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = (1, 50, 512)
N_SETS = max(COUNTS)
LANE_T = 1024  # more than 2 x 256 CUs: minimal9_launch takes the lane-per-hypothesis kernel


@pytest.fixture(scope="module")
def sets(rsdsfm):
    """N_SETS 9-point sets (q, u: [N][9][2]; alpha, alpha_k: [N][9]); the first six are degenerate"""
    rng = np.random.default_rng(20261019)
    frames = [rsdsfm.synth.make_config(cfg, seed=1000 + i, rows=96, cols=128) for i, cfg in enumerate((3, 1, 3, 1))]
    q, u, a, ak = (np.empty((N_SETS, 9, 2)), np.empty((N_SETS, 9, 2)), np.empty((N_SETS, 9)), np.empty((N_SETS, 9)))
    for i in range(N_SETS):
        d = frames[i % len(frames)]
        idx = rng.choice(len(d["q"]), 9, replace=False)
        q[i], u[i], a[i], ak[i] = d["q"][idx], d["u"][idx], d["alpha"][idx], d["alpha_k"][idx]
    # a repeated point (two equal rows of the 9x9 system), in two places
    for i, (dst, src) in ((0, (8, 0)), (1, (4, 3))):
        q[i, dst], u[i, dst], a[i, dst], ak[i, dst] = q[i, src], u[i, src], a[i, src], ak[i, src]
    # all-zero flow (three zero columns), with the frame's alpha and with alpha = 1
    u[2] = 0.0
    u[3] = 0.0
    a[3] = 1.0
    # nine collinear points: pixels of one image row (pix = column * rows + row), and a slanted line under the set's own flow
    d = frames[0]
    row = np.flatnonzero(d["pix"] % 96 == 40)[::13][:9]
    assert len(row) == 9
    q[4], u[4], a[4], ak[4] = d["q"][row], d["u"][row], d["alpha"][row], d["alpha_k"][row]
    t = np.linspace(-0.4, 0.4, 9)
    q[5] = np.stack([t, 0.5 * t + 0.05], axis=1)
    return q, u, a, ak


def _bits(x):
    """bit patterns with every NaN mapped to one value: NaNs compare as equal"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64).copy()
    b[np.isnan(x)] = np.uint64(0x7FF8000000000000)
    return b


@pytest.fixture(scope="module")
def lane_reference(rsdsfm, sets):
    """the lane-per-hypothesis kernel's outputs for all N_SETS sets, per use_alpha_k: computed once, shared, never modified"""
    import torch

    dev = torch.device("cuda", 0)
    q, u, a, ak = sets
    reps = LANE_T // N_SETS
    out = {}
    with rsdsfm.Solver(0) as s:
        dq, du, da, dak = (torch.from_numpy(np.ascontiguousarray(np.tile(x, (reps,) + (1,) * (x.ndim - 1)))).to(dev) for x in (q, u, a, ak))
        for use_k in (0, 1):
            hyp = torch.zeros(8 * LANE_T, dtype=torch.float64, device=dev)
            s.minimal9_dev(dq.data_ptr(), du.data_ptr(), da.data_ptr(), dak.data_ptr(), LANE_T, use_k, 0, hyp.data_ptr())
            s.synchronize()
            h = hyp.cpu().numpy().reshape(reps, N_SETS, 8)
            assert np.array_equal(_bits(h[0]), _bits(h[-1]))  # (a lane's result does not depend on where it ran)
            out[use_k] = h[0].copy()
            out[use_k].setflags(write=False)
    return out


@pytest.mark.parametrize("use_k", (0, 1))
@pytest.mark.parametrize("count", COUNTS)
def test_minimal9_wave_cores_and_lane_forms_bit_identical(rsdsfm, sets, lane_reference, count, use_k):
    import torch

    dev = torch.device("cuda", 0)
    q, u, a, ak = sets
    dq, du, da, dak = (torch.from_numpy(np.ascontiguousarray(x[:count])).to(dev) for x in (q, u, a, ak))
    res = {}
    with rsdsfm.Solver(0) as s:
        for cores in (1, 0):
            hyp = torch.zeros(8 * count, dtype=torch.float64, device=dev)
            probe = torch.zeros(4 * count, dtype=torch.float64, device=dev)
            s.minimal9_probe_dev(dq.data_ptr(), du.data_ptr(), da.data_ptr(), dak.data_ptr(), count, use_k, 0, cores, hyp.data_ptr(), probe.data_ptr())
            s.synchronize()
            res[cores] = (hyp.cpu().numpy().reshape(count, 8), probe.cpu().numpy().reshape(count, 4))
    ref = lane_reference[use_k][:count]
    for cores in (1, 0):
        h, p = res[cores]
        bad = np.flatnonzero((_bits(h) != _bits(ref)).any(axis=1))
        assert bad.size == 0, "wave form (cores %d) differs from the lane form at hypotheses %s: %s vs %s" % (cores, bad[:8], h[bad[:2]], ref[bad[:2]])
        assert (p[:, 0] >= 1).all() and (p[:, 0] <= 1000).all()
    assert np.array_equal(res[1][1][:, 0], res[0][1][:, 0]), "sweep counts differ between the cores and the standard functions"
    assert np.array_equal(res[1][1][:, 1], res[0][1][:, 1]), "rotation counts differ between the cores and the standard functions"
    assert np.array_equal(_bits(res[1][0]), _bits(res[0][0]))
