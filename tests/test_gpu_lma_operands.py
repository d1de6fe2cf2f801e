"""GPU: the staged operands of the analytic pixel pass (rsdsfm_set_lma_operands 0, the default: one thread per pixel loads q, u, alpha, alpha_k,
forms x y, x x + 1, y y + 1 and -- where every hypothesis carries the same k -- beta, and leaves a record in LDS that the pixel's lanes read;
mode 2: the same for every hypothesis count, where mode 0 keeps the per-lane loads for groups of few hypotheses)
return the bytes of the per-lane loads (mode 1) -- on fresh contexts with identical call histories and the same seeded inputs: every integer
and float of rsdsfm_frame_result, depth map, pose table, the refined inliers with their indices and scanlines; rsdsfm_ransac's counts, error
sums, best trial, mask, inverse depths and accepted steps; rsdsfm_lma_restarts and rsdsfm_lma_predict_stats.  Both library builds.  (The
pattern of tests/test_gpu_frame_predict.py.)

Shapes: 8 x 8 (fewer pixels than one tile), 61 x 97 (ragged last tile and last workgroup), 160 x 120 (several workgroups); 5, 43, 50 and 130
hypotheses (51, 5, 5 and 5 pixel slots; 130 = three hypothesis groups)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_hip = None


def _d2h(ptr, nbytes, dtype):
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so")
    out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
    if nbytes:
        assert _hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 2) == 0
    return out


def _record(r, dm, R, t, lists=True):
    m = int(r["num_inliers"])
    sm = r["refine_summary"]
    rec = (int(r["n"]), m, int(r["best_trial"]), bool(r["flipped"]), r["ransac_v"].tobytes(), r["ransac_w"].tobytes(), np.float64(r["ransac_k"]).tobytes(),
           r["v"].tobytes(), r["w"].tobytes(), np.float64(r["k"]).tobytes(), tuple(sorted((k, np.float64(v).tobytes()) for k, v in sm.items())),
           dm.cpu().numpy().tobytes(), R.cpu().numpy().tobytes(), t.cpu().numpy().tobytes())
    if lists:
        rec += (_d2h(r["d_inliers"], 24 * m, np.float64).tobytes(), _d2h(r["d_inlier_idx"], 8 * m, np.int64).tobytes(), _d2h(r["d_scanline"], 4 * m, np.int32).tobytes())
    return rec


_NAMES = ("n", "num_inliers", "best_trial", "flipped", "ransac_v", "ransac_w", "ransac_k", "v", "w", "k", "refine_summary", "depth_map", "pose_R", "pose_t",
          "d_inliers", "d_inlier_idx", "d_scanline")
_MODES = (1, 0, 2)  # (the per-lane loads first: the reference of the comparison)


@pytest.fixture(params=["reference", "fused"])
def arith(request):
    return request.param


def _solve_modes(rsdsfm, arith, frame, seeds, lm_arithmetic=0, **kw):
    """the same solves, in order, on a fresh context per mode; returns {mode: [record per solve]}, {mode: (lma_restarts, predict_stats) after the last}"""
    import torch

    dev = torch.device("cuda", 0)
    flow, rows, cols, K, gamma = frame
    img = torch.from_numpy(np.ascontiguousarray(flow)).to(dev)
    out, stats = {}, {}
    for mode in _MODES:
        recs = []
        with rsdsfm.Solver(0, arith=arith) as s:
            s.set_lma_operands(mode)
            if lm_arithmetic:
                s.set_lm_arithmetic(lm_arithmetic)
            for seed in seeds:
                dm = torch.full((cols, rows), -7.0, dtype=torch.float64, device=dev)
                R = torch.full((rows, 9), -7.0, dtype=torch.float64, device=dev)
                t = torch.full((rows, 3), -7.0, dtype=torch.float64, device=dev)
                r = s.solve_frame_dev(img.data_ptr(), rows, cols, K, gamma, dm.data_ptr(), R.data_ptr(), t.data_ptr(), seed=seed, **kw)
                s.synchronize()
                recs.append(_record(r, dm, R, t))
            stats[mode] = (tuple(s.lma_restarts()), tuple(s.lma_predict_stats()))
        out[mode] = recs
    return out, stats


def _frame(d, img=None):
    return (d["flow_img"] if img is None else img, d["rows"], d["cols"], d["K"], d["gamma"])


def _assert_same(res, what):
    out, stats = res
    for mode in (0, 2):
        assert len(out[mode]) == len(out[1])
        for i, (a, b) in enumerate(zip(out[mode], out[1])):
            for nm, x, y in zip(_NAMES, a, b):
                assert x == y, "%s: solve %d: %s differs between the staged operands (mode %d) and the per-lane loads" % (what, i, nm, mode)
        assert stats[mode] == stats[1], "%s: (lma_restarts, lma_predict_stats) %s in mode %d, %s per lane" % (what, stats[mode], mode, stats[1])


def test_fewer_pixels_than_one_tile(rsdsfm, arith):
    """8 x 8: 64 pixels, one workgroup per group whose only tile is ragged"""
    d = rsdsfm.synth.make_config(5, rows=8, cols=8)
    res = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), trials=8, tol=0.05)
    _assert_same(res, "8x8")


def test_ragged_last_tile_and_workgroup(rsdsfm, arith):
    """61 columns x 97 rows = 5917 pixels: no multiple of the pixel slots, of a tile or of the workgroups' chunk"""
    d = rsdsfm.synth.make_config(5, rows=97, cols=61)
    res = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), trials=16, tol=0.05)
    _assert_same(res, "61x97")
    assert all(rec[1] > 0 for rec in res[0][0])


@pytest.mark.parametrize("trials", [5, 43, 50, 130])
def test_hypothesis_counts(rsdsfm, arith, trials):
    """160 x 120, several workgroups: T = 5 (51 pixel slots: tiles of 4 rounds), 43 and 50 (5 slots: tiles of 50 rounds), 130 (three groups of
    44 hypotheses)"""
    d = rsdsfm.synth.make_config(5, rows=120, cols=160)
    res = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), trials=trials, tol=0.05)
    _assert_same(res, "160x120 T=%d" % trials)
    assert all(rec[1] > 0 for rec in res[0][0])
    assert res[1][0][1][0] >= trials  # (the own-iterate pass ran: its staged form was the one compared)


def test_count_only_pass(rsdsfm, arith):
    """tolerance 0.002 with the count-only form forced (rsdsfm_set_lm_arithmetic 2): the staged ransac_lma_own_kernel<false>"""
    d = rsdsfm.synth.make_config(5, rows=120, cols=160)
    res = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), lm_arithmetic=2, trials=50, tol=0.002)
    _assert_same(res, "count-only")
    assert all(rec[1] > 0 for rec in res[0][0])


def test_acceleration_mode(rsdsfm, arith):
    """k estimated per hypothesis (hypotheses without a real k: a NaN pose): no uniform k, so the 72-byte record and beta in the lanes"""
    d = rsdsfm.synth.make_config(5, rows=120, cols=160)
    res = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), trials=50, tol=0.05, use_acceleration_mode=True)
    _assert_same(res, "acceleration mode")
    assert all(rec[1] > 0 for rec in res[0][0])


def test_noise_free_flow(rsdsfm, arith):
    """noise-free: the inlier counts tie, the analytic run starts over on the iterate-by-iterate kernels -- in both modes alike"""
    d = rsdsfm.synth.make_config(2, rows=120, cols=160)
    res = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), trials=16, tol=0.05)
    _assert_same(res, "noise-free")
    assert all(rec[1] > 0 for rec in res[0][0])
    print("noise-free: (lma_restarts, predict_stats)", res[1][0])


def test_pixels_below_flow_threshold(rsdsfm, arith):
    """160 x 120 with a 20 x 15 hole of zero flow: the general flatten, so the two-iterate pass (ransac_lma_kernel<2, .>) on 18 900 pixels"""
    d = rsdsfm.synth.make_config(5, rows=120, cols=160)
    img = d["flow_img"].copy()
    img[40:55, 100:120] = 0.0
    res = _solve_modes(rsdsfm, arith, _frame(d, img), seeds=(1, 2, 3), trials=16, tol=0.05)
    _assert_same(res, "hole")
    assert all(rec[0] == 120 * 160 - 15 * 20 and rec[1] > 0 for rec in res[0][0])


def test_listed_pixels(rsdsfm, arith):
    """forward motion: the focus of expansion (v_x / v_z, v_y / v_z) = (0.067, 0.033) lies inside the frame, so the pixels around it are clamped
    (guard a) and go to the hypotheses' lists from both forms of the pass"""
    d = rsdsfm.synth.make_config(5, rows=120, cols=160, v=np.array([0.002, 0.001, 0.03]))
    res = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), trials=50, tol=0.05)
    _assert_same(res, "focus of expansion inside")
    assert all(rec[1] > 0 for rec in res[0][0])


_RANSAC_NAMES = ("num_inliers", "best_trial", "w", "v", "k", "inlier_error", "inlier_idx", "inliers", "alpha", "alpha_k", "mask", "inv_depth", "trial_count",
                 "trial_err", "trial_vel", "trial_steps")


@pytest.mark.parametrize("use_alpha_k", [0, 1])
@pytest.mark.parametrize("trials", [50, 130])
def test_ransac(rsdsfm, arith, trials, use_alpha_k):
    """rsdsfm_ransac on 160 x 120 (the two-iterate pass with error sums): the 64-byte record without the k estimation, the 72-byte one with it"""
    d = rsdsfm.synth.make_config(5, rows=120, cols=160)
    got = {}
    for mode in _MODES:
        with rsdsfm.Solver(0, arith=arith) as s:
            s.set_lma_operands(mode)
            rr = [s.ransac(d["q"], d["u"], d["alpha"], d["alpha_k"], use_alpha_k, trials, 0.05, seed=seed) for seed in (1, 2)]
            got[mode] = ([tuple(np.asarray(r[nm]).tobytes() for nm in _RANSAC_NAMES) for r in rr], tuple(s.lma_restarts()))
            assert all(r["num_inliers"] > 0 for r in rr)
    for mode in (0, 2):
        for i, (a, b) in enumerate(zip(got[mode][0], got[1][0])):
            for nm, x, y in zip(_RANSAC_NAMES, a, b):
                assert x == y, "rsdsfm_ransac T=%d use_alpha_k=%d: run %d: %s differs between the staged operands (mode %d) and the per-lane loads" % (trials, use_alpha_k, i, nm, mode)
        assert got[mode][1] == got[1][1]


def test_sequence_of_frames_three_lanes(rsdsfm, arith):
    """rsdsfm_solve_frames_dev with 3 lanes: the mode is copied to the lanes, and every pair returns the bytes of its single solve in mode 1"""
    import torch

    dev = torch.device("cuda", 0)
    frames = [rsdsfm.synth.make_config(5, rows=120, cols=160, seed=0x5EED0300 + i) for i in range(6)]
    seeds = [1 + i for i in range(len(frames))]
    kw = dict(trials=16, tol=0.05)
    imgs = [torch.from_numpy(f["flow_img"]).to(dev) for f in frames]

    def bufs(f):
        return (torch.full((f["cols"], f["rows"]), -7.0, dtype=torch.float64, device=dev), torch.full((f["rows"], 9), -7.0, dtype=torch.float64, device=dev),
                torch.full((f["rows"], 3), -7.0, dtype=torch.float64, device=dev))

    single = []
    with rsdsfm.Solver(0, arith=arith) as s:
        s.set_lma_operands(1)
        for f, im, seed in zip(frames, imgs, seeds):
            dm, R, t = bufs(f)
            r = s.solve_frame_dev(im.data_ptr(), f["rows"], f["cols"], f["K"], f["gamma"], dm.data_ptr(), R.data_ptr(), t.data_ptr(), seed=seed, **kw)
            s.synchronize()
            single.append(_record(r, dm, R, t, lists=False))
    stats = {}
    for mode in _MODES:
        with rsdsfm.Solver(0, arith=arith) as s:
            s.set_sequence_lanes(3)
            bb = [bufs(f) for f in frames]
            jobs = [dict(d_flow_img=im.data_ptr(), rows=f["rows"], cols=f["cols"], K=f["K"], gamma=f["gamma"], d_depth_map=b[0].data_ptr(), d_R=b[1].data_ptr(),
                         d_t=b[2].data_ptr()) for f, im, b in zip(frames, imgs, bb)]
            s.solve_frames_dev(jobs[:3], seeds[:3], **kw)  # (the lanes exist from here on: the switch below has to reach them)
            s.synchronize()
            s.set_lma_operands(mode)
            res = s.solve_frames_dev(jobs, seeds, **kw)
            s.synchronize()
            for i, r in enumerate(res):
                rec = _record(r, *bb[i], lists=False)
                for nm, x, y in zip(_NAMES, rec, single[i]):
                    assert x == y, "3 lanes, lma_operands %d: pair %d: %s differs from the single solve in mode 1" % (mode, i, nm)
            stats[mode] = (tuple(s.lma_restarts()), tuple(s.lma_predict_stats()))
    assert stats[0] == stats[1] == stats[2], stats


def test_mode_is_checked(rsdsfm):
    with rsdsfm.Solver(0) as s:
        with pytest.raises(Exception):
            s.set_lma_operands(3)
        with pytest.raises(Exception):
            s.set_lma_operands(-1)
        for mode in (2, 1, 0):
            s.set_lma_operands(mode)
