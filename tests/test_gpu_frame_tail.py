"""GPU: the frame solve's short launch tail (rsdsfm_set_frame_tail 0, the default: the refinement's output pass claims the depth-map
pixels, one kernel decides the sign of z and writes header, pose table and depth map) returns the bytes of the stage-by-stage launches
(mode 1) -- on fresh contexts with identical call histories and the same seeded inputs: depth map, pose table, every integer and float of
rsdsfm_frame_result, the refined inliers, their pixel indices and their scanlines.
(The RANSAC's dense rho and mask live in the context's frame arena and are not reachable through the C ABI; the RANSAC stages are the
same launches in both modes.)"""
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
    ml = m if lists else 0  # (lists = False: the device-resident lists are no longer this solve's)
    sm = r["refine_summary"]
    return (int(r["n"]), m, int(r["best_trial"]), bool(r["flipped"]), r["ransac_v"].tobytes(), r["ransac_w"].tobytes(), np.float64(r["ransac_k"]).tobytes(),
            r["v"].tobytes(), r["w"].tobytes(), np.float64(r["k"]).tobytes(), tuple(sorted((k, np.float64(v).tobytes()) for k, v in sm.items())),
            dm.cpu().numpy().tobytes(), R.cpu().numpy().tobytes(), t.cpu().numpy().tobytes(), _d2h(r["d_inliers"], 24 * ml, np.float64).tobytes(),
            _d2h(r["d_inlier_idx"], 8 * ml, np.int64).tobytes(), _d2h(r["d_scanline"], 4 * ml, np.int32).tobytes())


_NAMES = ("n", "num_inliers", "best_trial", "flipped", "ransac_v", "ransac_w", "ransac_k", "v", "w", "k", "refine_summary", "depth_map", "pose_R", "pose_t",
          "d_inliers", "d_inlier_idx", "d_scanline")


def _solve_both(rsdsfm, img_h, rows, cols, K, gamma, seeds, **kw):
    """the same solves (one per sampler seed, in order) on a fresh context per mode; returns {mode: [record per seed]}"""
    import torch

    dev = torch.device("cuda", 0)
    img = torch.from_numpy(np.ascontiguousarray(img_h)).to(dev)
    out = {}
    for mode in (0, 1):
        recs = []
        with rsdsfm.Solver(0) as s:
            s.set_frame_tail(mode)
            for seed in seeds:
                dm = torch.full((cols, rows), -7.0, dtype=torch.float64, device=dev)
                R = torch.full((rows, 9), -7.0, dtype=torch.float64, device=dev)
                t = torch.full((rows, 3), -7.0, dtype=torch.float64, device=dev)
                r = s.solve_frame_dev(img.data_ptr(), rows, cols, K, gamma, dm.data_ptr(), R.data_ptr(), t.data_ptr(), seed=seed, **kw)
                s.synchronize()
                recs.append(_record(r, dm, R, t))
        out[mode] = recs
    return out


def _assert_same(out, what):
    assert len(out[0]) == len(out[1])
    for i, (a, b) in enumerate(zip(out[0], out[1])):
        for nm, x, y in zip(_NAMES, a, b):
            assert x == y, "%s: solve %d: %s differs between the short tail and the stage-by-stage launches" % (what, i, nm)


def test_bench_configuration_1280x720(rsdsfm, big_config):
    """bench.py's headline: 1280x720 DeepFlow-like pair, T = 50, tol 0.05, 8 sampler seeds in a row on one context"""
    d = big_config(5)
    out = _solve_both(rsdsfm, d["flow_img"], d["rows"], d["cols"], d["K"], d["gamma"], seeds=range(1, 9), trials=50, tol=0.05)
    _assert_same(out, "1280x720")
    assert all(rec[1] > 0 for rec in out[0])


def test_1920x1080(rsdsfm):
    d = rsdsfm.synth.make_config(5, rows=1080, cols=1920)
    out = _solve_both(rsdsfm, d["flow_img"], d["rows"], d["cols"], d["K"], d["gamma"], seeds=(1, 2), trials=50, tol=0.05)
    _assert_same(out, "1920x1080")
    assert all(rec[1] > 0 for rec in out[0])


def test_ragged_size(rsdsfm):
    """37 columns x 53 rows: no multiple of any tile or workgroup"""
    d = rsdsfm.synth.make_config(5, rows=53, cols=37)
    out = _solve_both(rsdsfm, d["flow_img"], d["rows"], d["cols"], d["K"], d["gamma"], seeds=(1, 2, 3), trials=20, tol=0.05)
    _assert_same(out, "37x53")
    assert all(rec[1] > 0 for rec in out[0])


def test_pixels_below_flow_threshold(rsdsfm):
    """a hole without flow: the speculation on a dense frame fails and everything runs again on the real point count"""
    d = rsdsfm.synth.make_config(5, rows=130, cols=210)
    img = d["flow_img"].copy()
    img[40:70, 100:140] = 0.0
    out = _solve_both(rsdsfm, img, d["rows"], d["cols"], d["K"], d["gamma"], seeds=(1, 2, 3), trials=16, tol=0.05)
    _assert_same(out, "hole")
    assert all(rec[0] < d["rows"] * d["cols"] and rec[1] > 0 for rec in out[0])


def test_noise_free_flow(rsdsfm):
    """noise-free flow: the pick behind round 0 is undecided and the final stage runs twice"""
    d = rsdsfm.synth.make_config(2, rows=180, cols=320)
    out = _solve_both(rsdsfm, d["flow_img"], d["rows"], d["cols"], d["K"], d["gamma"], seeds=(1, 2, 3), trials=16, tol=0.05)
    _assert_same(out, "noise-free")
    assert all(rec[1] > 0 for rec in out[0])


def test_acceleration_mode(rsdsfm):
    d = rsdsfm.synth.make_config(5, rows=240, cols=320)
    out = _solve_both(rsdsfm, d["flow_img"], d["rows"], d["cols"], d["K"], d["gamma"], seeds=(1, 2, 3), trials=16, tol=0.05, use_acceleration_mode=True)
    _assert_same(out, "acceleration mode")
    assert all(rec[1] > 0 for rec in out[0])


def test_without_refinement(rsdsfm):
    """use_refinement = 0 keeps the stage-by-stage depth map in both modes"""
    d = rsdsfm.synth.make_config(5, rows=130, cols=210)
    out = _solve_both(rsdsfm, d["flow_img"], d["rows"], d["cols"], d["K"], d["gamma"], seeds=(1, 2), trials=16, tol=0.05, use_refinement=False)
    _assert_same(out, "no refinement")


FLIP_CASE = dict(cfg=3, rows=96, cols=160, trials=8, tol=0.004)  # the sampler seeds: see test_flip_branch


def _oracle_flipped(oracle, f, T, tol, seed):
    """the CPU oracle's whole chain on the frame (as __graft_entry__.smoke): is the mean z of the refined inliers negative?"""
    rows, K, gamma = f["rows"], f["K"], f["gamma"]
    qf, uf, qpx, fpx = oracle.flatten(f["flow_img"], *K, gamma)
    af, akf = oracle.get_alpha(fpx, rows, gamma), oracle.get_alpha_k(qpx, fpx, rows, gamma)
    ro = oracle.ransac(qf, uf, af, akf, False, T, tol, oracle.sample_indices(len(qf), T, seed), depth_mode=1)
    refo = oracle.refine(uf, ro["inliers"], ro["alpha"], ro["alpha_k"], ro["v"], ro["w"], ro["k"], False, 0, None)
    return bool(oracle.canonicalize_sign(refo["inliers"], refo["v"])[2])


def test_flip_branch(rsdsfm, oracle):
    """frames whose refined inliers have a negative mean z (main.cc:472-478: v and z change sign).  The sign of the minimal solver's v is
    the SVD's, so it varies with the sampler seed: the seeds are taken from the CPU oracle's chain, not from the code under test, and at
    least one of each kind must be among them"""
    f = rsdsfm.synth.make_config(FLIP_CASE["cfg"], rows=FLIP_CASE["rows"], cols=FLIP_CASE["cols"])
    T, tol = FLIP_CASE["trials"], FLIP_CASE["tol"]
    kinds = {}
    for seed in range(1, 40):
        kinds.setdefault(_oracle_flipped(oracle, f, T, tol, seed), seed)
        if len(kinds) == 2:
            break
    assert True in kinds, "the oracle found no sampler seed whose solve flips the sign"
    seeds = [kinds[True]] + ([kinds[False]] if False in kinds else [])
    out = _solve_both(rsdsfm, f["flow_img"], f["rows"], f["cols"], f["K"], f["gamma"], seeds=seeds, trials=T, tol=tol)
    _assert_same(out, "flip")
    assert out[0][0][3] is True, "the GPU solve of the oracle's flipped frame did not flip"
    if len(seeds) > 1:
        assert out[0][1][3] is False


def test_sequence_of_frames_four_lanes(rsdsfm):
    """rsdsfm_solve_frames_dev with 4 lanes: the mode is copied to the lanes, pair by pair the same bytes"""
    import torch

    dev = torch.device("cuda", 0)
    frames = [rsdsfm.synth.make_config((5, 3)[i % 2], rows=150, cols=260, seed=0x5EED0200 + i) for i in range(9)]
    out = {}
    for mode in (0, 1):
        with rsdsfm.Solver(0) as s:
            s.set_frame_tail(mode)
            s.set_sequence_lanes(4)
            imgs = [torch.from_numpy(f["flow_img"]).to(dev) for f in frames]
            dms = [torch.full((f["cols"], f["rows"]), -7.0, dtype=torch.float64, device=dev) for f in frames]
            Rs = [torch.full((f["rows"], 9), -7.0, dtype=torch.float64, device=dev) for f in frames]
            ts = [torch.full((f["rows"], 3), -7.0, dtype=torch.float64, device=dev) for f in frames]
            jobs = [dict(d_flow_img=im.data_ptr(), rows=f["rows"], cols=f["cols"], K=f["K"], gamma=f["gamma"], d_depth_map=dm.data_ptr(), d_R=R.data_ptr(),
                         d_t=t.data_ptr()) for f, im, dm, R, t in zip(frames, imgs, dms, Rs, ts)]
            recs = []
            for rep in range(2):
                res = s.solve_frames_dev(jobs, [1 + 10 * rep + i for i in range(len(jobs))], trials=16, tol=0.02)
                s.synchronize()
                # (a lane's device-resident lists are those of the LAST pair it solved: 4 lanes, the last 4 pairs)
                for i, r in enumerate(res):
                    recs.append(_record(r, dms[i], Rs[i], ts[i], lists=i >= len(res) - 4))
        out[mode] = recs
    _assert_same(out, "4 lanes")
