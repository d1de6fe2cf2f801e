"""GPU: whole clips through the solve (rsdsfm_solve_video_dev) -- the same fields as deep_flow_seq and the same results as
rsdsfm_solve_frames_dev on them (fresh contexts on both sides: some float diagnostics depend on a context's history), with caller
buffers or the library's ring, at any lane count; accurate on render_sequence; evaluate_real_sequence = evaluate_real_run per pair."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _scaled_motion(rsdsfm, rows, cols, K, gamma, target):
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    s = target / np.abs(f0).max()
    return v * s, w * s, k


def _record(r, dm, R, t):
    sm = r["refine_summary"]
    return (r["n"], r["num_inliers"], r["best_trial"], r["flipped"], r["ransac_v"].tobytes(), r["ransac_w"].tobytes(), float(r["ransac_k"]),
            r["v"].tobytes(), r["w"].tobytes(), float(r["k"]), sm["num_iterations"], sm["num_successful_steps"], sm["termination"],
            sm["final_cost"], dm.cpu().numpy().tobytes(), R.cpu().numpy().tobytes(), t.cpu().numpy().tobytes())


def _buffers(torch, dev, n, rows, cols):
    return ([torch.zeros(rows * cols, dtype=torch.float64, device=dev) for _ in range(n)],
            [torch.zeros((rows, 9), dtype=torch.float64, device=dev) for _ in range(n)],
            [torch.zeros((rows, 3), dtype=torch.float64, device=dev) for _ in range(n)])


@pytest.fixture(scope="module")
def clip(rsdsfm):
    rows, cols, gamma = 120, 160, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, 3.0)
    frames, _, _ = rsdsfm.synth.render_sequence(7, rows, cols, K, v, w, k, gamma, seed=21)
    return frames, rows, cols, K, gamma


def _video(rsdsfm, torch, clip, seeds, batch, lanes, with_flows):
    frames, rows, cols, K, gamma = clip
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)] if with_flows else None
    dms, Rs, ts = _buffers(torch, dev, n, rows, cols)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        s.set_flow_batch(batch)
        s.set_sequence_lanes(lanes)
        res = s.solve_video_dev([f.data_ptr() for f in d_frames], rows, cols, 3, K, gamma, [m.data_ptr() for m in dms], seeds=seeds,
                                d_flows=[f.data_ptr() for f in d_flows] if with_flows else None, d_R=[r.data_ptr() for r in Rs],
                                d_t=[t.data_ptr() for t in ts], trials=20)
        s.synchronize()
    recs = [_record(r, dms[i], Rs[i], ts[i]) for i, r in enumerate(res)]
    return recs, [f.cpu().numpy() for f in d_flows] if with_flows else None


@pytest.fixture(scope="module")
def reference(rsdsfm, clip):
    """deep_flow_seq of the clip, and solve_frames_dev on those fields (a fresh context, default lanes)"""
    import torch

    frames, rows, cols, K, gamma = clip
    n = len(frames) - 1
    seeds = [3 + 5 * i for i in range(n)]
    with rsdsfm.Solver(0) as s:
        flows = s.deep_flow_seq(frames)
    dev = torch.device("cuda", 0)
    d_flows = [torch.from_numpy(f).to(dev) for f in flows]
    dms, Rs, ts = _buffers(torch, dev, n, rows, cols)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        jobs = [dict(d_flow_img=d_flows[i].data_ptr(), rows=rows, cols=cols, K=K, gamma=gamma, d_depth_map=dms[i].data_ptr(), d_R=Rs[i].data_ptr(),
                     d_t=ts[i].data_ptr()) for i in range(n)]
        res = s.solve_frames_dev(jobs, seeds, trials=20)
        s.synchronize()
    return flows, seeds, [_record(r, dms[i], Rs[i], ts[i]) for i, r in enumerate(res)]


def test_caller_flows_equal_deep_flow_seq_and_solve_frames(rsdsfm, clip, reference):
    import torch

    flows, seeds, want = reference
    got, got_flows = _video(rsdsfm, torch, clip, seeds, batch=4, lanes=0, with_flows=True)
    for p in range(len(flows)):
        assert np.array_equal(got_flows[p].view(np.uint64), flows[p].view(np.uint64)), p
    assert got == want, [i for i in range(len(want)) if got[i] != want[i]]
    assert min(r[1] for r in got) > 0


def test_library_ring_with_ragged_tail(rsdsfm, clip, reference):
    """7 frames = 6 pairs at B = 4 (one full batch, then a ragged batch of 2 that reuses the ring), and at B = 2 with NULL flows"""
    import torch

    _, seeds, want = reference
    for batch in (4, 2):
        got, _ = _video(rsdsfm, torch, clip, seeds, batch=batch, lanes=0, with_flows=False)
        assert got == want, (batch, [i for i in range(len(want)) if got[i] != want[i]])


@pytest.mark.parametrize("lanes", [1, 3])
def test_lanes_change_nothing(rsdsfm, clip, reference, lanes):
    import torch

    _, seeds, want = reference
    got, _ = _video(rsdsfm, torch, clip, seeds, batch=3, lanes=lanes, with_flows=False)
    assert got == want


def test_accuracy_on_a_rendered_clip(rsdsfm):
    """every pair of a 5-frame render_sequence clip at 640x480: rotation error <= 10 % of |w|, direction of v within 5 degrees (the
    bounds of test_gpu_flow.py::test_end_to_end_flow_into_the_solve)"""
    import torch

    rows, cols, gamma = 480, 640, 0.8
    K = rsdsfm.synth.INTRINSICS["galaxy_vga"]
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, 5.0)
    frames, _, _ = rsdsfm.synth.render_sequence(5, rows, cols, K, v, w, k, gamma, seed=3)
    dev = torch.device("cuda", 0)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    dms = [torch.empty(rows * cols, dtype=torch.float64, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        res = s.solve_video_dev([f.data_ptr() for f in d_frames], rows, cols, 3, K, gamma, [m.data_ptr() for m in dms], trials=50, tol=0.05)
        s.synchronize()
    for p, r in enumerate(res):
        w_err, v_err = rsdsfm.velocity_errors(r["w"], r["v"], w, v)
        print("pair %d: inliers %d of %d, w error %.3g (|w| %.3g), v error %.3f deg" % (p, r["num_inliers"], r["n"], w_err, np.linalg.norm(w), np.degrees(v_err)))
        assert w_err <= 0.1 * np.linalg.norm(w), p
        assert np.degrees(v_err) <= 5.0, p


def test_evaluate_real_sequence_is_evaluate_real_run_per_pair(rsdsfm, tmp_path):
    rows, cols, gamma = 240, 320, 0.95
    K = tuple(x * 0.5 for x in rsdsfm.synth.INTRINSICS["galaxy_vga"])
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, 4.0)
    frames, _, _ = rsdsfm.synth.render_sequence(4, rows, cols, K, v, w, k, gamma, seed=9)
    prefix = str(tmp_path / "clip") + "/"
    os.makedirs(prefix)
    for j, f in enumerate(frames):
        rsdsfm.formats.write_png(prefix + "frame%d.png" % (j + 1), f)
    with rsdsfm.Solver(0) as s:
        out = rsdsfm.evaluate.evaluate_real_sequence(s, prefix, camera=K, gamma=gamma, out_dir=str(tmp_path / "out"), trials=20)
        assert len(out) == 3
        for p in range(3):
            ref = rsdsfm.evaluate.evaluate_real_run(s, frames[p], None, camera=K, gamma=gamma, frame2=frames[p + 1], trials=20)
            for key in ("flow", "depth_map", "depth_est", "backprojection", "coords", "R", "t", "v", "w"):
                assert np.array_equal(np.asarray(out[p][key]), np.asarray(ref[key])), (p, key)
            assert out[p]["k"] == ref["k"] and out[p]["num_inliers"] == ref["num_inliers"], p
            for name in ("optical_flow.png", "MinimalDepth.png", "rs_image.png", "backprojection.png", "point_cloud.ply"):
                assert os.path.exists(str(tmp_path / "out" / str(p) / name)), (p, name)
    lines = open(str(tmp_path / "out" / "poses.csv")).read().splitlines()
    assert lines[0] == "pair,v_x,v_y,v_z,w_x,w_y,w_z,k,inliers" and len(lines) == 4
    assert [int(ln.split(",")[0]) for ln in lines[1:]] == [0, 1, 2]
    assert [int(ln.split(",")[-1]) for ln in lines[1:]] == [o["num_inliers"] for o in out]
