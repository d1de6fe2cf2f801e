"""GPU: whole clips through the dense rectifier (rsdsfm_rectify_dense_video_dev).  Per pair it returns what rsdsfm_solve_video_dev returns, and
its dense image, mask and filled depth are the bytes of rsdsfm_rectify_dense_frame_dev on results[p]'s depth map and pose table -- at every
batch size and lane count, for BGR and gray clips; and the evaluation drivers' dense option."""
import os

import numpy as np
import pytest

import flow_spec_numpy as spec
from test_gpu_video import _record, _scaled_motion

pytestmark = pytest.mark.gpu

TRIALS = 20
TOL = 0.001  # this clip's pairs then keep 1305 .. 2204 of their 3072 pixels (at the default 0.05 all of them: nothing to fill)


@pytest.fixture(scope="module")
def clip(rsdsfm):
    rows, cols, gamma = 48, 64, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, 2.0)
    frames, _, _ = rsdsfm.synth.render_sequence(5, rows, cols, K, v, w, k, gamma, seed=21)
    gray = np.stack([spec.gray(f).astype(np.uint8) for f in frames])
    return dict(frames=frames, gray=gray, rows=rows, cols=cols, K=K, gamma=gamma, seeds=[3 + 5 * i for i in range(len(frames) - 1)])


def _reference(rsdsfm, torch, clip, frames):
    """existing calls only: solve_video_dev on a fresh context, then the single-frame dense call per pair on that pair's depth map and pose table"""
    rows, cols, K, gamma = clip["rows"], clip["cols"], clip["K"], clip["gamma"]
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    ch = 1 if frames[0].ndim == 2 else 3
    d_frames = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    mk = lambda shape, dtype: [torch.zeros(shape, dtype=dtype, device=dev) for _ in range(n)]
    dms, Rs, ts = mk((rows * cols,), torch.float64), mk((rows, 9), torch.float64), mk((rows, 3), torch.float64)
    ptrs = lambda a: [x.data_ptr() for x in a]
    out = []
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        s.set_flow_batch(4)
        res = s.solve_video_dev(ptrs(d_frames), rows, cols, ch, K, gamma, ptrs(dms), seeds=clip["seeds"], d_R=ptrs(Rs), d_t=ptrs(ts), trials=TRIALS, tol=TOL)
        s.synchronize()
        for p, r in enumerate(res):
            dense, mask = torch.full_like(d_frames[p], 77), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
            filled = torch.full((rows * cols,), np.nan, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            s.rectify_dense_frame_dev(d_frames[p].data_ptr(), ch, dms[p].data_ptr(), Rs[p].data_ptr(), ts[p].data_ptr(), K, rows, cols, dense.data_ptr(),
                                      mask.data_ptr(), filled.data_ptr())
            s.synchronize()
            out.append(dict(record=_record(r, dms[p], Rs[p], ts[p]), images=tuple(x.cpu().numpy().tobytes() for x in (dense, mask, filled)),
                            mask=mask.cpu().numpy(), holes=float((dms[p] == 0).double().mean())))
    return out


@pytest.fixture(scope="module")
def reference(rsdsfm, clip):
    import torch

    return _reference(rsdsfm, torch, clip, clip["frames"])


@pytest.fixture(scope="module")
def reference_gray(rsdsfm, clip):
    import torch

    return _reference(rsdsfm, torch, clip, clip["gray"])


def _video(rsdsfm, torch, clip, frames, batch, lanes, own_tables, **kw):
    rows, cols, K, gamma = clip["rows"], clip["cols"], clip["K"], clip["gamma"]
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    ch = 1 if frames[0].ndim == 2 else 3
    d_frames = [torch.from_numpy(np.ascontiguousarray(f)).to(dev) for f in frames]
    mk = lambda shape, dtype, fill: [torch.full(shape, fill, dtype=dtype, device=dev) for _ in range(n)]
    dms, Rs, ts = mk((rows * cols,), torch.float64, 0.0), mk((rows, 9), torch.float64, 0.0), mk((rows, 3), torch.float64, 0.0)
    dense, masks = mk(tuple(d_frames[0].shape), torch.uint8, 77), mk((rows, cols), torch.uint8, 77)
    filled = mk((rows * cols,), torch.float64, np.nan)
    ptrs = lambda a: [x.data_ptr() for x in a]
    args = dict(d_masks=ptrs(masks), d_filled=ptrs(filled), seeds=clip["seeds"], trials=TRIALS, tol=TOL)
    if own_tables:
        args.update(d_R=ptrs(Rs), d_t=ptrs(ts))
    args.update(kw)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        s.set_flow_batch(batch)
        s.set_sequence_lanes(lanes)
        res = s.rectify_dense_video_dev(ptrs(d_frames), rows, cols, ch, K, gamma, ptrs(dms), ptrs(dense), **args)
        # (no synchronize: every output is complete when the call returns)
        return [dict(record=_record(r, dms[i], Rs[i], ts[i]), images=tuple(x.cpu().numpy().tobytes() for x in (dense[i], masks[i], filled[i])))
                for i, r in enumerate(res)]


def _same(got, want, own_tables):
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert g["images"] == w["images"], (p, [i for i in range(3) if g["images"][i] != w["images"][i]])
        assert (g["record"] == w["record"]) if own_tables else (g["record"][:-2] == w["record"][:-2]), p
        assert w["record"][1] > 0 and 0.0 < w["holes"] < 1.0 and w["mask"].any(), p  # inliers, holes for the fill to close, valid pixels


@pytest.mark.parametrize("batch,lanes,own_tables", [(1, 1, True), (2, 3, False), (8, 1, False), (8, 3, True)])
def test_clip_equals_the_single_frame_calls(rsdsfm, clip, reference, batch, lanes, own_tables):
    import torch

    _same(_video(rsdsfm, torch, clip, clip["frames"], batch, lanes, own_tables), reference, own_tables)


@pytest.mark.parametrize("batch,lanes", [(2, 3), (8, 1)])
def test_gray_clip(rsdsfm, clip, reference_gray, batch, lanes):
    import torch

    _same(_video(rsdsfm, torch, clip, clip["gray"], batch, lanes, True), reference_gray, True)


def test_argument_errors(rsdsfm, clip):
    import torch

    rows, cols, K, gamma = clip["rows"], clip["cols"], clip["K"], clip["gamma"]
    dev = torch.device("cuda", 0)
    n = 2
    d_frames = [torch.from_numpy(f).to(dev) for f in clip["frames"][:n + 1]]
    dms = [torch.zeros(rows * cols, dtype=torch.float64, device=dev) for _ in range(n)]
    dense = [torch.zeros_like(d_frames[0]) for _ in range(n)]
    masks = [torch.zeros((rows, cols), dtype=torch.uint8, device=dev) for _ in range(n)]
    ptrs = lambda a: [x.data_ptr() for x in a]
    with rsdsfm.Solver(0) as s:
        call = lambda frames=d_frames, channels=3, out=ptrs(dense), k=n, **kw: s.rectify_dense_video_dev(
            ptrs(frames), rows, cols, channels, K, gamma, ptrs(dms[:k]), out[:k], trials=TRIALS, **kw)
        with pytest.raises(rsdsfm.RsdsfmError, match="rectify video: null device pointer"):
            call(out=[dense[0].data_ptr(), 0])
        with pytest.raises(rsdsfm.RsdsfmError, match="rectify video: null device pointer"):
            call(d_masks=[masks[0].data_ptr(), 0])
        with pytest.raises(rsdsfm.RsdsfmError, match="rectify video: channels must be 1 or 3"):
            call(channels=2)
        with pytest.raises(rsdsfm.RsdsfmError, match="rectify video: nframes must be >= 2"):
            call(frames=d_frames[:1], k=0)
        with pytest.raises(rsdsfm.RsdsfmError):
            call(out=[dense[0].data_ptr(), d_frames[1].data_ptr()])  # pair 1 writes over its own frame
        for bad in (dict(mode=2), dict(q5_mode=7), dict(iterations=17)):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        assert len(call()) == n  # the same arguments without a fault go through


def test_drivers_write_the_dense_files_on_request(rsdsfm, clip, tmp_path):
    """evaluate_real_sequence(dense=True) writes rectified_dense.png and rectified_dense_mask.png per pair and returns the single-frame call's
    arrays; without it the directory listing is what it was"""
    import torch

    rows, cols, K, gamma = clip["rows"], clip["cols"], clip["K"], clip["gamma"]
    frames = clip["frames"][:3]
    today = {"optical_flow.png", "MinimalDepth.png", "rs_image.png", "backprojection.png", "point_cloud.ply"}
    with rsdsfm.Solver(0) as s:
        plain = rsdsfm.evaluate.evaluate_real_sequence(s, frames, camera=K, gamma=gamma, trials=TRIALS, out_dir=str(tmp_path / "plain"))
    with rsdsfm.Solver(0) as s:
        dense = rsdsfm.evaluate.evaluate_real_sequence(s, frames, camera=K, gamma=gamma, trials=TRIALS, out_dir=str(tmp_path / "dense"), dense=True)
    assert set(os.listdir(str(tmp_path / "plain"))) == {"0", "1", "poses.csv"} == set(os.listdir(str(tmp_path / "dense")))
    dev = torch.device("cuda", 0)
    for p in range(2):
        assert set(os.listdir(str(tmp_path / "plain" / str(p)))) == today
        assert set(os.listdir(str(tmp_path / "dense" / str(p)))) == today | {"rectified_dense.png", "rectified_dense_mask.png"}
        assert "dense_image" not in plain[p] and set(dense[p]) == set(plain[p]) | {"dense_image", "dense_mask"}
        for key in ("depth_map", "gs_image", "backprojection", "R", "t"):
            assert np.array_equal(dense[p][key], plain[p][key]), key
        o = dense[p]
        with rsdsfm.Solver(0) as s:
            img, mask = s.rectify_dense(frames[p], o["depth_map"], o["R"], o["t"], K)
        assert np.array_equal(img, o["dense_image"]) and np.array_equal(mask, o["dense_mask"]) and mask.any()
        assert np.array_equal(rsdsfm.formats.read_png(str(tmp_path / "dense" / str(p) / "rectified_dense.png")), img)
        assert np.array_equal(rsdsfm.formats.read_png(str(tmp_path / "dense" / str(p) / "rectified_dense_mask.png"), grayscale=True), mask * 255)
    with rsdsfm.Solver(0) as s:  # the single-pair driver: the same arrays and files
        one = rsdsfm.evaluate.evaluate_real_run(s, frames[0], None, camera=K, gamma=gamma, frame2=frames[1], trials=TRIALS, out_dir=str(tmp_path / "one"), dense=True)
    assert np.array_equal(one["dense_image"], dense[0]["dense_image"]) and np.array_equal(one["dense_mask"], dense[0]["dense_mask"])
    assert set(os.listdir(str(tmp_path / "one"))) == today | {"rectified_dense.png", "rectified_dense_mask.png"}
