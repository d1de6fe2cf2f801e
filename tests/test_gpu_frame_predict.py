"""GPU: the own-iterate pixel pass of a frame solve's RANSAC (rsdsfm_set_frame_predict 0, the default: the solver workgroups predict at
which iterate each hypothesis' depth solve ends and the pass fuses that iterate's score alone) and its inverted form (mode 2: every
hypothesis mispredicted, so every score comes from the scoring pass) return the bytes of the two-iterate pass (mode 1) -- on fresh contexts
with identical call histories and the same seeded inputs: depth map, pose table, every integer and float of rsdsfm_frame_result, and the
first m entries of the refined inliers, their pixel indices and their scanlines.  Both library builds.  (The pattern of
tests/test_gpu_frame_handoff.py.)"""
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


@pytest.fixture(params=["reference", "fused"])
def arith(request):
    return request.param


def _solve_modes(rsdsfm, arith, frame, seeds, lm_arithmetic=0, **kw):
    """the same solves, in order, on a fresh context per mode; returns {mode: [record per solve]}, {mode: [predict_stats after each solve]}"""
    import torch

    dev = torch.device("cuda", 0)
    flow, rows, cols, K, gamma = frame
    img = torch.from_numpy(np.ascontiguousarray(flow)).to(dev)
    out, stats = {}, {}
    for mode in (1, 0, 2):
        recs, st = [], []
        with rsdsfm.Solver(0, arith=arith) as s:
            s.set_frame_predict(mode)
            if lm_arithmetic:
                s.set_lm_arithmetic(lm_arithmetic)
            for seed in seeds:
                dm = torch.full((cols, rows), -7.0, dtype=torch.float64, device=dev)
                R = torch.full((rows, 9), -7.0, dtype=torch.float64, device=dev)
                t = torch.full((rows, 3), -7.0, dtype=torch.float64, device=dev)
                r = s.solve_frame_dev(img.data_ptr(), rows, cols, K, gamma, dm.data_ptr(), R.data_ptr(), t.data_ptr(), seed=seed, **kw)
                s.synchronize()
                recs.append(_record(r, dm, R, t))
                st.append(s.lma_predict_stats())
        out[mode], stats[mode] = recs, st
    return out, stats


def _frame(d, img=None):
    return (d["flow_img"] if img is None else img, d["rows"], d["cols"], d["K"], d["gamma"])


def _assert_same(out, what):
    for mode in (0, 2):
        assert len(out[mode]) == len(out[1])
        for i, (a, b) in enumerate(zip(out[mode], out[1])):
            for nm, x, y in zip(_NAMES, a, b):
                assert x == y, "%s: solve %d: %s differs between frame_predict %d and the two-iterate pass" % (what, i, nm, mode)


def _per_solve(st):
    """(hypotheses, hits) of each solve from the running totals"""
    return [(b[0] - a[0], b[1] - a[1]) for a, b in zip([(0, 0)] + st[:-1], st)]


def test_fewer_pixels_than_the_lattice(rsdsfm, arith):
    """8 x 8: the lattice is the whole frame, 64 of the 192 lattice lanes hold a pixel"""
    d = rsdsfm.synth.make_config(5, rows=8, cols=8)
    out, stats = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), trials=8, tol=0.05)
    _assert_same(out, "8x8")
    assert stats[1][-1] == (0, 0) and stats[0][-1][0] >= 8  # (mode 1 never runs the own-iterate pass; mode 0 ran it)


def test_ragged_size(rsdsfm, arith):
    """61 columns x 97 rows: no multiple of the flatten's tile, of the pass's pixel slots or of the lattice"""
    d = rsdsfm.synth.make_config(5, rows=97, cols=61)
    out, stats = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), trials=16, tol=0.05)
    _assert_same(out, "61x97")
    assert all(rec[1] > 0 for rec in out[0])


_COUNTS = {}


def _counts_case(rsdsfm, arith, trials):
    """160 x 120 DeepFlow-like, sampler seeds 1, 2, 3 (chosen before any run), solved once per (build, T) and shared by the two tests below"""
    if (arith, trials) not in _COUNTS:
        d = rsdsfm.synth.make_config(5, rows=120, cols=160)
        _COUNTS[(arith, trials)] = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), trials=trials, tol=0.05)
    return _COUNTS[(arith, trials)]


@pytest.mark.parametrize("trials", [5, 50, 64, 100])
def test_hypothesis_counts(rsdsfm, arith, trials):
    """T = 5 (51 pixel slots), 50 (the bench's), 64 (P = 4, no idle lane), 100 (two hypothesis groups): the bytes of mode 1"""
    out, stats = _counts_case(rsdsfm, arith, trials)
    _assert_same(out, "160x120 T=%d" % trials)
    assert all(rec[1] > 0 for rec in out[0])
    assert stats[1][-1] == (0, 0)  # (mode 1 never runs the own-iterate pass)


@pytest.mark.parametrize("trials", [5, 50, 64, 100])
def test_predict_stats(rsdsfm, arith, trials):
    """rsdsfm_lma_predict_stats on the same solves: in mode 0 at least T - 1 of the T hypotheses of every solve end where predicted; in
    mode 2 (the prediction inverted, the pass's scores discarded) none does.

    Measured (MI355X), T = 50, sampler seeds 1, 2, 3: mode 0 (50, 49), (50, 50), (50, 50).  Hypothesis 11 of sampler seed 1 ends after ONE step
    on all 19 200 pixels and after two on the lattice: its costs before / after the solve stand at 100.07 : 1 on all pixels (the function
    tolerance puts the boundary between one and two steps at 100 : 1) and at 108.9 : 1 on the lattice; the CPU oracle alone says the same.
    Mode 2 takes no score from the pass, so that hypothesis -- for which the inverted prediction is the right one -- goes to the scoring
    pass with the others."""
    out, stats = _counts_case(rsdsfm, arith, trials)
    per0, per2 = _per_solve(stats[0]), _per_solve(stats[2])
    print("T = %d: (hypotheses, ended where predicted) per solve: mode 0 %s, mode 2 %s" % (trials, per0, per2))
    for h, e in per0:
        assert h == trials and e >= trials - 1, per0
    for h, e in per2:
        assert h == trials and e == 0, per2


def test_count_only_pass(rsdsfm, arith):
    """tolerance 0.002 with the count-only form forced (rsdsfm_set_lm_arithmetic 2): ransac_lma_own_kernel<false>, the lazy error sums behind it"""
    d = rsdsfm.synth.make_config(5, rows=120, cols=160)
    out, stats = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), lm_arithmetic=2, trials=50, tol=0.002)
    _assert_same(out, "count-only")
    assert all(rec[1] > 0 for rec in out[0])
    assert stats[0][-1][0] >= 50  # (the own-iterate pass ran)


def test_acceleration_mode(rsdsfm, arith):
    """k estimated by the minimal solver (the k estimation in front of the SVD, hypotheses without a real k) and refined"""
    d = rsdsfm.synth.make_config(5, rows=120, cols=160)
    out, stats = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), trials=50, tol=0.05, use_acceleration_mode=True)
    _assert_same(out, "acceleration mode")
    assert all(rec[1] > 0 for rec in out[0])
    assert stats[0][-1][0] >= 50  # (the own-iterate pass ran)


def test_noise_free_flow(rsdsfm, arith):
    """noise-free: every hypothesis ends after three accepted steps, so everything is predicted 2 and scored by the scoring pass, as in mode 1"""
    d = rsdsfm.synth.make_config(2, rows=120, cols=160)
    out, stats = _solve_modes(rsdsfm, arith, _frame(d), seeds=(1, 2, 3), trials=16, tol=0.05)
    _assert_same(out, "noise-free")
    assert all(rec[1] > 0 for rec in out[0])


def test_pixels_below_flow_threshold(rsdsfm, arith):
    """160 x 120 with a 20 x 15 hole of zero flow: the frame is not dense, so its RANSAC runs behind the general flatten and takes the two-iterate
    pass in every mode -- only the first solve's discarded speculation on a dense frame went through the solver's launch"""
    d = rsdsfm.synth.make_config(5, rows=120, cols=160)
    img = d["flow_img"].copy()
    img[40:55, 100:120] = 0.0
    out, stats = _solve_modes(rsdsfm, arith, _frame(d, img), seeds=(1, 2, 3), trials=16, tol=0.05)
    _assert_same(out, "hole")
    assert all(rec[0] == 120 * 160 - 15 * 20 and rec[1] > 0 for rec in out[0])
    print("hole: predict_stats per solve, mode 0:", _per_solve(stats[0]))
    assert stats[0][-1][0] <= 16, stats[0]


def test_sequence_of_frames_three_lanes(rsdsfm, arith):
    """rsdsfm_solve_frames_dev with 3 lanes: the mode is copied to the lanes, every pair returns the bytes of its single solve in mode 1, and the
    counters are summed over the lanes"""
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
        s.set_frame_predict(1)
        for f, im, seed in zip(frames, imgs, seeds):
            dm, R, t = bufs(f)
            r = s.solve_frame_dev(im.data_ptr(), f["rows"], f["cols"], f["K"], f["gamma"], dm.data_ptr(), R.data_ptr(), t.data_ptr(), seed=seed, **kw)
            s.synchronize()
            single.append(_record(r, dm, R, t, lists=False))
    for mode in (0, 2):
        with rsdsfm.Solver(0, arith=arith) as s:
            s.set_frame_predict(mode)
            s.set_sequence_lanes(3)
            bb = [bufs(f) for f in frames]
            jobs = [dict(d_flow_img=im.data_ptr(), rows=f["rows"], cols=f["cols"], K=f["K"], gamma=f["gamma"], d_depth_map=b[0].data_ptr(), d_R=b[1].data_ptr(),
                         d_t=b[2].data_ptr()) for f, im, b in zip(frames, imgs, bb)]
            res = s.solve_frames_dev(jobs, seeds, **kw)
            s.synchronize()
            for i, r in enumerate(res):
                rec = _record(r, *bb[i], lists=False)
                for nm, x, y in zip(_NAMES, rec, single[i]):
                    assert x == y, "3 lanes, frame_predict %d: pair %d: %s differs from the single solve in mode 1" % (mode, i, nm)
            h, e = s.lma_predict_stats()
            assert h == 16 * len(frames), (mode, h, e)
            assert 0 <= e <= h, (mode, h, e)
            if mode == 0:  # (at least T - 1 of every pair's T hypotheses)
                assert e >= h - len(frames), (h, e)
