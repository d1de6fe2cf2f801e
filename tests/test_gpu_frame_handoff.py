"""GPU: the frame solve's direct hand-off (rsdsfm_set_frame_handoff 0, the default: the final stage leaves block-local inlier lists and the
refinement's first pass finds the pixel of every rank in them itself) returns the bytes of the compaction launch (mode 1) -- on fresh contexts
with identical call histories and the same seeded inputs: depth map, pose table, every integer and float of rsdsfm_frame_result, and the first
m entries of the refined inliers, their pixel indices and their scanlines.  (The pattern of tests/test_gpu_frame_tail.py.)"""
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


def _record(r, dm, R, t):
    m = int(r["num_inliers"])
    sm = r["refine_summary"]
    return (int(r["n"]), m, int(r["best_trial"]), bool(r["flipped"]), r["ransac_v"].tobytes(), r["ransac_w"].tobytes(), np.float64(r["ransac_k"]).tobytes(),
            r["v"].tobytes(), r["w"].tobytes(), np.float64(r["k"]).tobytes(), tuple(sorted((k, np.float64(v).tobytes()) for k, v in sm.items())),
            dm.cpu().numpy().tobytes(), R.cpu().numpy().tobytes(), t.cpu().numpy().tobytes(), _d2h(r["d_inliers"], 24 * m, np.float64).tobytes(),
            _d2h(r["d_inlier_idx"], 8 * m, np.int64).tobytes(), _d2h(r["d_scanline"], 4 * m, np.int32).tobytes())


_NAMES = ("n", "num_inliers", "best_trial", "flipped", "ransac_v", "ransac_w", "ransac_k", "v", "w", "k", "refine_summary", "depth_map", "pose_R", "pose_t",
          "d_inliers", "d_inlier_idx", "d_scanline")


def _solve_both(rsdsfm, frames, seeds, **kw):
    """the same solves, in order -- solve i is frames[i % len(frames)] with sampler seed seeds[i] -- on a fresh context per mode; a frame is
    (flow image, rows, cols, K, gamma).  Returns {mode: [record per solve]}"""
    import torch

    dev = torch.device("cuda", 0)
    imgs = [torch.from_numpy(np.ascontiguousarray(f[0])).to(dev) for f in frames]
    out = {}
    for mode in (0, 1):
        recs = []
        with rsdsfm.Solver(0) as s:
            s.set_frame_handoff(mode)
            for i, seed in enumerate(seeds):
                img, (_, rows, cols, K, gamma) = imgs[i % len(frames)], frames[i % len(frames)]
                dm = torch.full((cols, rows), -7.0, dtype=torch.float64, device=dev)
                R = torch.full((rows, 9), -7.0, dtype=torch.float64, device=dev)
                t = torch.full((rows, 3), -7.0, dtype=torch.float64, device=dev)
                r = s.solve_frame_dev(img.data_ptr(), rows, cols, K, gamma, dm.data_ptr(), R.data_ptr(), t.data_ptr(), seed=seed, **kw)
                s.synchronize()
                recs.append(_record(r, dm, R, t))
        out[mode] = recs
    return out


def _frame(d, img=None):
    return (d["flow_img"] if img is None else img, d["rows"], d["cols"], d["K"], d["gamma"])


def _assert_same(out, what):
    assert len(out[0]) == len(out[1])
    for i, (a, b) in enumerate(zip(out[0], out[1])):
        for nm, x, y in zip(_NAMES, a, b):
            assert x == y, "%s: solve %d: %s differs between the direct hand-off and the compaction launch" % (what, i, nm)


def test_ragged_size(rsdsfm):
    """37 columns x 53 rows, T = 20: no multiple of any tile, and the final stage's blocks are shorter than the refinement's 512-rank windows"""
    d = rsdsfm.synth.make_config(5, rows=53, cols=37)
    out = _solve_both(rsdsfm, [_frame(d)], seeds=(1, 2, 3), trials=20, tol=0.05)
    _assert_same(out, "37x53")
    assert all(rec[1] > 0 for rec in out[0])


def test_pixels_below_flow_threshold(rsdsfm):
    """210 x 130 with a 40 x 30 hole of zero flow: the speculation on a dense frame fails and everything runs again on the real point count"""
    d = rsdsfm.synth.make_config(5, rows=130, cols=210)
    img = d["flow_img"].copy()
    img[40:70, 100:140] = 0.0
    out = _solve_both(rsdsfm, [_frame(d, img)], seeds=(1, 2, 3), trials=16, tol=0.05)
    _assert_same(out, "hole")
    assert all(rec[0] == d["rows"] * d["cols"] - 40 * 30 and rec[1] > 0 for rec in out[0])


def test_noise_free_flow(rsdsfm):
    """320 x 180 noise-free: the pick behind round 0 is undecided, the speculated final stage and first pass leave at once, the final stage runs twice"""
    d = rsdsfm.synth.make_config(2, rows=180, cols=320)
    out = _solve_both(rsdsfm, [_frame(d)], seeds=(1, 2, 3), trials=16, tol=0.05)
    _assert_same(out, "noise-free")
    assert all(rec[1] > 0 for rec in out[0])


def test_acceleration_mode(rsdsfm):
    """k refined (NP = 7): the later passes read alpha and alpha_k by rank, which the first pass now writes"""
    d = rsdsfm.synth.make_config(5, rows=240, cols=320)
    out = _solve_both(rsdsfm, [_frame(d)], seeds=(1, 2, 3), trials=16, tol=0.05, use_acceleration_mode=True)
    _assert_same(out, "acceleration mode")
    assert all(rec[1] > 0 for rec in out[0])


def test_gathered_flow(rsdsfm):
    """flow_index_mode gathered: the flow of rank i is the flow of its pixel"""
    d = rsdsfm.synth.make_config(5, rows=240, cols=320)
    out = _solve_both(rsdsfm, [_frame(d)], seeds=(1, 2, 3), trials=16, tol=0.05, flow_index_mode=rsdsfm.FLOW_GATHERED)
    _assert_same(out, "gathered")
    assert all(rec[1] > 0 for rec in out[0])


OUTLIER_CASE = dict(rows=240, cols=320, noise_px=0.03, outliers=0.40, data_seed=0x5EED0405, trials=48, tol=0.002, seeds=(1, 2, 3))


def test_forty_percent_outliers(rsdsfm, oracle):
    """40 % outliers at tolerance 0.002: the ranks fall far behind the pixel indices and a 512-rank window of the first pass spans several of the
    final stage's blocks.  The inlier count must stay inside (0.3 n, 0.8 n), so that the case cannot pass by being all-inlier: checked on the
    CPU oracle's RANSAC for the sampler seeds used (with 0.3 px of noise the tolerance keeps under a quarter of the pixels, hence 0.03 px; with
    40 % outliers one 9-point sample in a hundred is clean, hence 48 trials)"""
    C = OUTLIER_CASE
    d = rsdsfm.synth.make_config(5, rows=C["rows"], cols=C["cols"])
    v, w, k = rsdsfm.synth.default_motion()
    img, _ = rsdsfm.synth.make_flow(C["rows"], C["cols"], d["K"], v, w, k, d["gamma"], C["noise_px"], C["outliers"], C["data_seed"])
    n = C["rows"] * C["cols"]
    qf, uf, qpx, fpx = oracle.flatten(img, *d["K"], d["gamma"])
    af, akf = oracle.get_alpha(fpx, C["rows"], d["gamma"]), oracle.get_alpha_k(qpx, fpx, C["rows"], d["gamma"])
    assert len(qf) == n
    m_oracle = [int(oracle.ransac(qf, uf, af, akf, False, C["trials"], C["tol"], oracle.sample_indices(n, C["trials"], seed), depth_mode=1)["num_inliers"])
                for seed in C["seeds"]]
    assert all(0.3 * n < m < 0.8 * n for m in m_oracle), m_oracle
    out = _solve_both(rsdsfm, [_frame(d, img)], seeds=C["seeds"], trials=C["trials"], tol=C["tol"])
    _assert_same(out, "40 % outliers")
    assert all(0.3 * n < rec[1] < 0.8 * n for rec in out[0]), [rec[1] for rec in out[0]]
    assert [rec[1] for rec in out[0]] == m_oracle


def test_first_size_with_two_windows_per_block(rsdsfm):
    """726 x 724 = 525,624 points: the first size above 2048 x 256, where a block of the final stage covers 512 pixels in two windows"""
    d = rsdsfm.synth.make_config(5, rows=724, cols=726)
    assert d["rows"] * d["cols"] == 525624 > 2048 * 256
    out = _solve_both(rsdsfm, [_frame(d)], seeds=(1,), trials=8, tol=0.05)
    _assert_same(out, "726x724")
    assert out[0][0][1] > 0


def test_eight_solves_alternating_two_sizes(rsdsfm):
    """eight solves in a row on one context, alternating two sizes: stale counts or lists of the previous solve would show"""
    a = rsdsfm.synth.make_config(5, rows=240, cols=320)
    b = rsdsfm.synth.make_config(3, rows=131, cols=211)
    out = _solve_both(rsdsfm, [_frame(a), _frame(b)], seeds=range(1, 9), trials=16, tol=0.02)
    _assert_same(out, "alternating sizes")
    assert all(rec[1] > 0 for rec in out[0])
    assert [rec[0] for rec in out[0]] == [240 * 320, 131 * 211] * 4
