"""GPU: the checked DeepFlow pair (rsdsfm_deep_flow_checked_dev) on a rendered occlusion (synth.render_occluded_pair, 96 x 128): its two
fields are rsdsfm_deep_flow_dev's, its mask / masked field / count the definition's (tests/flow_check_spec_numpy.py) on them; chained into
the solve, a rejected pixel carries no depth; evaluate_real_run(check_flow=True) is that chain, and its default is what it was."""
import os

import numpy as np
import pytest

import flow_check_cases as cases
import flow_check_spec_numpy as spec

pytestmark = pytest.mark.gpu

ROWS, COLS, GAMMA = 96, 128, 0.8
K = (0.75 * COLS, 0.75 * COLS, 0.5 * COLS, 0.5 * ROWS)


@pytest.fixture(scope="module")
def scene(rsdsfm):
    """the pair, the two plain fields (a fresh context) and the spec's outputs on them"""
    img1, img2, occluded, block, far = cases.occluded_scene(rsdsfm.synth, ROWS, COLS)
    with rsdsfm.Solver(0) as s:
        fwd, bwd = s.deep_flow(img1, img2), s.deep_flow(img2, img1)
    return dict(img1=img1, img2=img2, occluded=occluded, far=far, fwd=fwd, bwd=bwd, out=spec.flow_check(fwd, bwd))


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_checked_pair_is_two_flows_and_the_spec(rsdsfm, scene, arith):
    want = scene["out"]
    with rsdsfm.Solver(0, arith=arith) as s:
        got = s.deep_flow_checked(scene["img1"], scene["img2"])
    assert _same(got["bwd"], scene["bwd"])
    assert np.array_equal(got["mask"], want["mask"]) and got["count"] == want["count"]
    assert _same(got["flow"], want["masked"])
    keep = want["mask"].astype(bool)
    assert _same(got["flow"][keep], scene["fwd"][keep])  # the unmasked field under the mask
    # what the CPU test measures on the float32 flow spec holds here too (the fields are the spec's bit for bit: tests/test_gpu_flow.py)
    assert 1.0 - keep[scene["occluded"]].mean() >= 0.776 - 0.05 and keep[scene["far"]].mean() >= 1.0 - 0.05


def test_other_parameters_and_the_context_owned_backward_buffer(rsdsfm, scene):
    import torch

    dev = torch.device("cuda", 0)
    want = spec.flow_check(scene["fwd"], scene["bwd"], a1=0.0, a2=0.05)
    assert want["count"] < scene["out"]["count"]
    d1, d2 = torch.from_numpy(scene["img1"]).to(dev), torch.from_numpy(scene["img2"]).to(dev)
    flow = torch.full((ROWS, COLS, 2), np.nan, dtype=torch.float64, device=dev)
    mask = torch.full((ROWS, COLS), 77, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        s.deep_flow_checked_dev(d1.data_ptr(), d2.data_ptr(), ROWS, COLS, 3, flow.data_ptr(), mask.data_ptr(), a1=0.0, a2=0.05)  # no d_bwd, no d_count
        s.synchronize()
        assert np.array_equal(mask.cpu().numpy(), want["mask"]) and _same(flow.cpu().numpy(), want["masked"])
        # the plain call on the same context is undisturbed
        plain = torch.empty_like(flow)
        s.deep_flow_dev(d1.data_ptr(), d2.data_ptr(), ROWS, COLS, 3, plain.data_ptr())
        s.synchronize()
        assert _same(plain.cpu().numpy(), scene["fwd"])
        with pytest.raises(rsdsfm.RsdsfmError):
            s.deep_flow_checked_dev(d1.data_ptr(), d2.data_ptr(), ROWS, COLS, 3, flow.data_ptr(), mask.data_ptr() + 2)
        with pytest.raises(rsdsfm.RsdsfmError):
            s.deep_flow_checked_dev(d1.data_ptr(), d2.data_ptr(), ROWS, COLS, 3, flow.data_ptr(), mask.data_ptr(), d_bwd=flow.data_ptr())
        with pytest.raises(rsdsfm.RsdsfmError):
            s.deep_flow_checked_dev(d1.data_ptr(), d2.data_ptr(), ROWS, COLS, 3, flow.data_ptr(), mask.data_ptr(), a1=-1.0)


def test_chained_into_the_solve_rejected_pixels_carry_no_depth(rsdsfm, scene):
    import torch

    dev = torch.device("cuda", 0)
    d1, d2 = torch.from_numpy(scene["img1"]).to(dev), torch.from_numpy(scene["img2"]).to(dev)
    flow = torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev)
    mask = torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    dm = torch.full((ROWS * COLS,), np.nan, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        s.deep_flow_checked_dev(d1.data_ptr(), d2.data_ptr(), ROWS, COLS, 3, flow.data_ptr(), mask.data_ptr(), d_count=count.data_ptr())
        r = s.solve_frame_dev(flow.data_ptr(), ROWS, COLS, K, GAMMA, dm.data_ptr(), trials=20, seed=4)  # same stream, same buffer, no wait between
        s.synchronize()
    m = mask.cpu().numpy().astype(bool)
    depth = dm.cpu().numpy().reshape(COLS, ROWS).T  # the device map is column-major
    assert not depth[~m].any() and (~m).sum() > 300
    assert 0 < r["num_inliers"] <= r["n"] <= int(count.cpu()[0]) == scene["out"]["count"]
    assert depth[m].any()


def test_evaluate_real_run_checked_is_the_manual_chain(rsdsfm, scene, tmp_path):
    import torch

    ev = rsdsfm.evaluate
    with rsdsfm.Solver(0) as s:
        plain = ev.evaluate_real_run(s, scene["img1"], None, camera=K, gamma=GAMMA, frame2=scene["img2"], trials=20, seed=4, out_dir=str(tmp_path / "plain"))
    with rsdsfm.Solver(0) as s:
        out = ev.evaluate_real_run(s, scene["img1"], None, camera=K, gamma=GAMMA, frame2=scene["img2"], trials=20, seed=4, out_dir=str(tmp_path / "checked"),
                                   check_flow=True)
        with pytest.raises(ValueError):
            ev.evaluate_real_run(s, scene["img1"], scene["fwd"], camera=K, gamma=GAMMA, check_flow=True)
    # the default: its keys and files, and the unmasked field
    assert "flow_mask" not in plain and "flow_consistent" not in plain and _same(plain["flow"], scene["fwd"])
    assert set(out) == set(plain) | {"flow_mask", "flow_consistent"}
    files = set(os.listdir(str(tmp_path / "plain")))
    assert files == {"optical_flow.png", "MinimalDepth.png", "rs_image.png", "backprojection.png", "point_cloud.ply"}
    assert set(os.listdir(str(tmp_path / "checked"))) == files | {"flow_mask.png"}
    assert np.array_equal(rsdsfm.formats.read_png(str(tmp_path / "checked" / "flow_mask.png"), grayscale=True), out["flow_mask"] * 255)
    # the manual chain on a fresh context
    dev = torch.device("cuda", 0)
    d1, d2 = torch.from_numpy(scene["img1"]).to(dev), torch.from_numpy(scene["img2"]).to(dev)
    flow = torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev)
    mask = torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
    dm = torch.empty(ROWS * COLS, dtype=torch.float64, device=dev)
    R, t = torch.empty(ROWS * 9, dtype=torch.float64, device=dev), torch.empty(ROWS * 3, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        s.deep_flow_checked_dev(d1.data_ptr(), d2.data_ptr(), ROWS, COLS, 3, flow.data_ptr(), mask.data_ptr())
        r = s.solve_frame_dev(flow.data_ptr(), ROWS, COLS, K, GAMMA, dm.data_ptr(), R.data_ptr(), t.data_ptr(), trials=20, seed=4)
        s.synchronize()
    assert np.array_equal(out["flow_mask"], mask.cpu().numpy()) and out["flow_consistent"] == scene["out"]["count"]
    assert _same(out["flow"], flow.cpu().numpy()) and _same(out["flow"], scene["out"]["masked"])
    assert _same(out["depth_map"], dm.cpu().numpy().reshape(COLS, ROWS).T) and _same(out["R"].reshape(-1), R.cpu().numpy()) and _same(out["t"].reshape(-1), t.cpu().numpy())
    assert out["num_inliers"] == r["num_inliers"] and out["n"] == r["n"] and out["k"] == r["k"]
    assert out["v"].tobytes() == r["v"].tobytes() and out["w"].tobytes() == r["w"].tobytes()


def test_evaluate_real_sequence_checked_is_evaluate_real_run_checked_per_pair(rsdsfm, tmp_path):
    """three frames with a block that moves on its own: per pair every output of evaluate_real_run(..., check_flow=True), dense outputs
    included, and its files; the default call returns neither mask nor count"""
    ev, synth = rsdsfm.evaluate, rsdsfm.synth
    v, w, k = synth.default_motion()
    f0, _ = synth.make_flow(ROWS, COLS, K, v, w, k, GAMMA, _model_only=True)
    s3 = 3.0 / np.abs(f0).max()
    frames, _, _ = synth.render_sequence(3, ROWS, COLS, K, v * s3, w * s3, k, GAMMA, seed=21)
    frames = frames.copy()
    for j in range(3):
        frames[j, 30 + 5 * j:58 + 5 * j, 48 - 8 * j:84 - 8 * j] = frames[0, 5:33, 90:126][:, :, ::-1]
    seeds = [4, 9]
    with rsdsfm.Solver(0) as s:
        outs = ev.evaluate_real_sequence(s, frames, camera=K, gamma=GAMMA, trials=20, seeds=seeds, out_dir=str(tmp_path / "seq"), dense=True, check_flow=True)
        plain = ev.evaluate_real_sequence(s, frames, camera=K, gamma=GAMMA, trials=20, seeds=seeds)
    assert len(outs) == 2 and all("flow_mask" not in o and "flow_consistent" not in o for o in plain)
    for p in range(2):
        with rsdsfm.Solver(0) as s:
            ref = ev.evaluate_real_run(s, frames[p], None, camera=K, gamma=GAMMA, frame2=frames[p + 1], trials=20, seed=seeds[p], dense=True, check_flow=True)
        assert set(outs[p]) == set(ref), p
        for key in ("flow", "flow_mask", "depth_map", "depth_est", "gs_image", "backprojection", "coords", "R", "t", "v", "w", "dense_image", "dense_mask"):
            assert np.array_equal(np.asarray(outs[p][key]), np.asarray(ref[key])), (p, key)
        assert outs[p]["flow_consistent"] == ref["flow_consistent"] == int(ref["flow_mask"].sum()) < ROWS * COLS, p
        assert outs[p]["k"] == ref["k"] and outs[p]["num_inliers"] == ref["num_inliers"] and outs[p]["n"] == ref["n"], p
        assert not np.array_equal(outs[p]["flow"], plain[p]["flow"]), p  # (the masked field, not the plain one)
        names = set(os.listdir(str(tmp_path / "seq" / str(p))))
        assert names == {"optical_flow.png", "MinimalDepth.png", "rs_image.png", "backprojection.png", "point_cloud.ply", "rectified_dense.png",
                         "rectified_dense_mask.png", "flow_mask.png"}, p
        assert np.array_equal(rsdsfm.formats.read_png(str(tmp_path / "seq" / str(p) / "flow_mask.png"), grayscale=True), outs[p]["flow_mask"] * 255)
