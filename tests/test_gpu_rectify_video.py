"""GPU: whole clips through the rectifier (rsdsfm_rectify_video_dev).  Per pair it returns what rsdsfm_solve_video_dev returns, and its
four image outputs are the bytes of deep_flow_dev -> solve_frame_dev -> rectify_frame_dev on a fresh context -- with caller buffers or
the library's ring and lane tables, at every batch size and lane count, for BGR and for gray clips; evaluate_real_run on a gray pair."""
import numpy as np
import pytest

import flow_spec_numpy as spec
from test_gpu_video import _record, _scaled_motion

pytestmark = pytest.mark.gpu

TRIALS = 20


@pytest.fixture(scope="module")
def clip(rsdsfm):
    """the clip of tests/test_gpu_video.py (every pair of it has inliers: asserted there and again here), and its gray version"""
    rows, cols, gamma = 120, 160, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, 3.0)
    frames, _, _ = rsdsfm.synth.render_sequence(7, rows, cols, K, v, w, k, gamma, seed=21)
    gray = np.stack([spec.gray(f).astype(np.uint8) for f in frames])
    return dict(frames=frames, gray=gray, rows=rows, cols=cols, K=K, gamma=gamma, seeds=[3 + 5 * i for i in range(len(frames) - 1)])


def _per_pair(rsdsfm, torch, clip, frames, also_replicated=False):
    """existing single-pair calls only, on a fresh context: per pair the record of test_gpu_video.py and the rectifier's four outputs"""
    rows, cols, K, gamma = clip["rows"], clip["cols"], clip["K"], clip["gamma"]
    dev = torch.device("cuda", 0)
    gray = frames[0].ndim == 2
    d_frames = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    out = []
    with rsdsfm.Solver(0) as s:
        for p in range(len(frames) - 1):
            flow = torch.empty((rows, cols, 2), dtype=torch.float64, device=dev)
            dm, R, t = torch.zeros(rows * cols, dtype=torch.float64, device=dev), torch.zeros((rows, 9), dtype=torch.float64, device=dev), torch.zeros((rows, 3), dtype=torch.float64, device=dev)
            prev = torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
            gs, fixed = torch.zeros_like(d_frames[p]), torch.zeros_like(d_frames[p])
            c3 = torch.zeros((rows, cols, 3), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            s.deep_flow_dev(d_frames[p].data_ptr(), d_frames[p + 1].data_ptr(), rows, cols, 1 if gray else 3, flow.data_ptr())
            r = s.solve_frame_dev(flow.data_ptr(), rows, cols, K, gamma, dm.data_ptr(), R.data_ptr(), t.data_ptr(), trials=TRIALS, seed=clip["seeds"][p])
            rectify = s.rectify_gray_frame_dev if gray else s.rectify_frame_dev
            rectify(r["d_inliers"], r["num_inliers"], d_frames[p].data_ptr(), dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, rows, cols, prev.data_ptr(),
                    gs.data_ptr(), fixed.data_ptr(), c3.data_ptr(), offset=1)
            s.synchronize()
            one = dict(record=_record(r, dm, R, t), flow=flow.cpu().numpy(), images=tuple(x.cpu().numpy().tobytes() for x in (prev, gs, fixed, c3)),
                       gs=gs.cpu().numpy())
            if also_replicated:  # the BGR rectifier on (g, g, g), from the same solve: the gray outputs are its channel 0
                rep = d_frames[p][:, :, None].expand(rows, cols, 3).contiguous()
                prev3, gs3, fixed3, c33 = torch.zeros_like(prev), torch.zeros_like(rep), torch.zeros_like(rep), torch.zeros_like(c3)
                s.rectify_frame_dev(r["d_inliers"], r["num_inliers"], rep.data_ptr(), dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, rows, cols, prev3.data_ptr(),
                                    gs3.data_ptr(), fixed3.data_ptr(), c33.data_ptr(), offset=1)
                s.synchronize()
                one["replicated"] = tuple(x.cpu().numpy().tobytes() for x in (prev3, gs3[:, :, 0].contiguous(), fixed3[:, :, 0].contiguous(), c33))
            out.append(one)
    return out


@pytest.fixture(scope="module")
def reference(rsdsfm, clip):
    import torch

    return _per_pair(rsdsfm, torch, clip, clip["frames"])


@pytest.fixture(scope="module")
def reference_gray(rsdsfm, clip):
    import torch

    return _per_pair(rsdsfm, torch, clip, clip["gray"], also_replicated=True)


def _video(rsdsfm, torch, clip, frames, batch, lanes, own_buffers, **kw):
    """rectify_video_dev on a fresh context; own_buffers: caller flows and pose tables, else the library's ring and lane tables"""
    rows, cols, K, gamma = clip["rows"], clip["cols"], clip["K"], clip["gamma"]
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    ch = 1 if frames[0].ndim == 2 else 3
    d_frames = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    mk = lambda shape, dtype, fill: [torch.full(shape, fill, dtype=dtype, device=dev) for _ in range(n)]
    dms, Rs, ts = mk((rows * cols,), torch.float64, 0.0), mk((rows, 9), torch.float64, 0.0), mk((rows, 3), torch.float64, 0.0)
    flows = mk((rows, cols, 2), torch.float64, np.nan)
    prevs, c3s = mk((rows, cols), torch.uint8, 77), mk((rows, cols, 3), torch.float32, np.nan)
    img_shape = (rows, cols) if ch == 1 else (rows, cols, 3)
    gss, fixeds = mk(img_shape, torch.uint8, 77), mk(img_shape, torch.uint8, 77)
    ptrs = lambda a: [x.data_ptr() for x in a]
    args = dict(d_coords=ptrs(c3s), seeds=clip["seeds"], trials=TRIALS, offset=1)
    if own_buffers:
        args.update(d_flows=ptrs(flows), d_R=ptrs(Rs), d_t=ptrs(ts))
    args.update(kw)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        s.set_flow_batch(batch)
        s.set_sequence_lanes(lanes)
        res = s.rectify_video_dev(ptrs(d_frames), rows, cols, ch, K, gamma, ptrs(dms), ptrs(prevs), ptrs(gss), ptrs(fixeds), **args)
        # (no synchronize: every output is complete when the call returns)
        out = [dict(record=_record(r, dms[i], Rs[i], ts[i]), flow=flows[i].cpu().numpy(), gs=gss[i].cpu().numpy(),
                    images=tuple(x.cpu().numpy().tobytes() for x in (prevs[i], gss[i], fixeds[i], c3s[i]))) for i, r in enumerate(res)]
    return out


def _non_black(img):
    """cv::norm(pixel) > 15 (camera.cc:694); a gray value g is the pixel (g, g, g)"""
    sq = img.astype(np.int64) ** 2
    return (sq.sum(axis=2) if img.ndim == 3 else 3 * sq) > 225


def _same(got, want, own_buffers):
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert g["images"] == w["images"], (p, [i for i in range(4) if g["images"][i] != w["images"][i]])
        if own_buffers:
            assert np.array_equal(g["flow"].view(np.uint64), w["flow"].view(np.uint64)), p
            assert g["record"] == w["record"], p
        else:  # no caller tables: the record without them
            assert g["record"][:-2] == w["record"][:-2], p
        assert g["record"][1] > 0 and _non_black(g["gs"]).any(), p  # inliers, and a non-black pixel in the global-shutter image


def test_clip_equals_the_single_pair_calls(rsdsfm, clip, reference):
    import torch

    _same(_video(rsdsfm, torch, clip, clip["frames"], batch=4, lanes=0, own_buffers=True), reference, True)


@pytest.mark.parametrize("batch,lanes", [(2, 0), (4, 1), (4, 3)])
def test_ring_lane_tables_batches_and_lanes_change_nothing(rsdsfm, clip, reference, batch, lanes):
    """d_flows = NULL (the ring) and d_R = d_t = NULL (a scratch table per lane): 6 pairs in batches of 2, and of 4 + 2 on 1 and 3 lanes"""
    import torch

    _same(_video(rsdsfm, torch, clip, clip["frames"], batch=batch, lanes=lanes, own_buffers=False), reference, False)


def test_gray_clip(rsdsfm, clip, reference, reference_gray):
    """channels = 1: the flow takes a gray frame as is and converts BGR with the integer formula of flow_spec_numpy.gray, so the fields
    and the solves are the BGR clip's (which carries its inlier condition over); the images are rectify_gray_frame_dev's, and channel 0
    of rectify_frame_dev's on the replicated frame"""
    import torch

    for p, (g, b) in enumerate(zip(reference_gray, reference)):
        assert np.array_equal(g["flow"].view(np.uint64), b["flow"].view(np.uint64)), p
        assert g["record"] == b["record"], p
        assert g["images"] == g["replicated"], (p, [i for i in range(4) if g["images"][i] != g["replicated"][i]])
        assert g["images"][0] == b["images"][0] and g["images"][3] == b["images"][3], p  # depth image and world points: no channel in them
    _same(_video(rsdsfm, torch, clip, clip["gray"], batch=4, lanes=0, own_buffers=True), reference_gray, True)
    _same(_video(rsdsfm, torch, clip, clip["gray"], batch=2, lanes=3, own_buffers=False), reference_gray, False)


def test_argument_errors(rsdsfm, clip):
    import torch

    rows, cols, K, gamma = clip["rows"], clip["cols"], clip["K"], clip["gamma"]
    dev = torch.device("cuda", 0)
    n = 2
    d_frames = [torch.from_numpy(f).to(dev) for f in clip["frames"][:n + 1]]
    dms = [torch.zeros(rows * cols, dtype=torch.float64, device=dev) for _ in range(n)]
    prevs = [torch.zeros((rows, cols), dtype=torch.uint8, device=dev) for _ in range(n)]
    gss, fixeds = [torch.zeros_like(d_frames[0]) for _ in range(n)], [torch.zeros_like(d_frames[0]) for _ in range(n)]
    ptrs = lambda a: [x.data_ptr() for x in a]
    with rsdsfm.Solver(0) as s:
        call = lambda frames=d_frames, channels=3, gs=ptrs(gss), fixed=ptrs(fixeds), k=n, **kw: s.rectify_video_dev(
            ptrs(frames), rows, cols, channels, K, gamma, ptrs(dms[:k]), ptrs(prevs[:k]), gs[:k], fixed[:k], trials=TRIALS, **kw)
        with pytest.raises(rsdsfm.RsdsfmError):
            call(channels=2)
        with pytest.raises(rsdsfm.RsdsfmError):
            call(frames=d_frames[:1], k=0)  # one frame: no pair
        with pytest.raises(rsdsfm.RsdsfmError):
            call(gs=[gss[0].data_ptr(), 0])
        with pytest.raises(rsdsfm.RsdsfmError):
            call(fixed=[fixeds[0].data_ptr(), gss[1].data_ptr()])  # pair 1: both images in one buffer
        with pytest.raises(rsdsfm.RsdsfmError):
            call(offset=-1)
        with pytest.raises(rsdsfm.RsdsfmError):
            call(mode=2)
        with pytest.raises(rsdsfm.RsdsfmError):
            call(q5_mode=7)
        assert len(call()) == n  # the same arguments without a fault go through


def test_evaluate_real_run_on_a_gray_pair(rsdsfm, clip, tmp_path):
    """2-D frames go to the gray rectifier: (rows, cols) images, every array equal to the run on the replicated BGR pair (whose integer
    gray conversion gives g back exactly), the images in channel 0; with out_dir the point cloud takes the replicated gray as colour"""
    import os

    rows, cols, K, gamma = clip["rows"], clip["cols"], clip["K"], clip["gamma"]
    g1, g2 = clip["gray"][0], clip["gray"][1]
    rep = lambda g: np.repeat(g[:, :, None], 3, axis=2)
    with rsdsfm.Solver(0) as s:
        out = rsdsfm.evaluate.evaluate_real_run(s, g1, None, camera=K, gamma=gamma, frame2=g2, trials=TRIALS, out_dir=str(tmp_path / "gray"))
    with rsdsfm.Solver(0) as s:
        ref = rsdsfm.evaluate.evaluate_real_run(s, rep(g1), None, camera=K, gamma=gamma, frame2=rep(g2), trials=TRIALS)
    assert out["gs_image"].shape == (rows, cols) and out["backprojection"].shape == (rows, cols)
    for key in ("flow", "depth_map", "depth_est", "coords", "R", "t", "v", "w"):
        assert np.array_equal(np.asarray(out[key]), np.asarray(ref[key])), key
    assert out["k"] == ref["k"] and out["num_inliers"] == ref["num_inliers"] > 0
    assert np.array_equal(out["gs_image"], ref["gs_image"][:, :, 0]) and np.array_equal(out["backprojection"], ref["backprojection"][:, :, 0])
    assert _non_black(out["gs_image"]).any()
    for name in ("optical_flow.png", "MinimalDepth.png", "rs_image.png", "backprojection.png", "point_cloud.ply"):
        assert os.path.exists(str(tmp_path / "gray" / name)), name
    with rsdsfm.Solver(0) as s:
        seq = rsdsfm.evaluate.evaluate_real_sequence(s, clip["gray"][:3], camera=K, gamma=gamma, trials=TRIALS)
    assert seq[0]["gs_image"].shape == (rows, cols)
    for key in ("flow", "depth_map", "depth_est", "gs_image", "backprojection", "coords", "R", "t", "v", "w"):
        assert np.array_equal(np.asarray(seq[0][key]), np.asarray(out[key])), key
