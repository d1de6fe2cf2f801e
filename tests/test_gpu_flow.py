"""GPU: the DeepFlow front end (include/rsdsfm_flow.h) -- bit for bit the numpy spec (tests/flow_spec_numpy.py), deterministic, the
same in both library builds and through both entry forms; accurate on rendered pairs; end to end into the solve and through
evaluate_real_run."""
import ctypes as C
import os

import numpy as np
import pytest

import flow_spec_numpy as S

pytestmark = pytest.mark.gpu

NONDEFAULT = dict(fixed_point_iterations=2, sor_iterations=7, downscale=0.8)


def _pair(rows, cols, seed):
    """frame 1 and a smoothly moved frame 2 (synth.render_pair at a small size, motion scaled to ~2 px)"""
    import rsdsfm

    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, 0.8, _model_only=True)
    s = 2.0 / np.abs(f0).max()
    a, b, _, _ = rsdsfm.synth.render_pair(rows, cols, K, v * s, w * s, k, 0.8, seed=seed)
    return a, b


def _scaled_motion(rsdsfm, rows, cols, K, gamma, target=5.0):
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    s = target / np.abs(f0).max()
    return v * s, w * s, k


@pytest.fixture(scope="module")
def solver(rsdsfm):
    with rsdsfm.Solver(0) as s:
        yield s


@pytest.mark.parametrize("rows,cols", [(37, 53), (60, 96), (96, 128), (120, 160)])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("params", [None, NONDEFAULT], ids=["default", "nondefault"])
def test_bit_identical_to_spec(solver, rows, cols, channels, params):
    a, b = _pair(rows, cols, seed=rows + cols)
    if channels == 1:
        a, b = a[..., 1].copy(), b[..., 1].copy()
    got = solver.deep_flow(a, b, params)
    want = S.deep_flow(a, b, **(params or {}))
    assert got.shape == (rows, cols, 2) and got.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.abs(got - want).max()
    assert np.abs(got).max() > 0.01  # something moved (2 x 7 iterations on 37 x 53 move little)


def test_entry_forms_builds_and_repeats_agree(rsdsfm, solver):
    import torch

    a, b = _pair(120, 160, seed=5)
    ref = solver.deep_flow(a, b)
    assert np.array_equal(solver.deep_flow(a, b).view(np.uint64), ref.view(np.uint64))  # two calls, same bits
    dev = torch.device("cuda", 0)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    df = torch.full((120, 160, 2), np.nan, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    solver.deep_flow_dev(da.data_ptr(), db.data_ptr(), 120, 160, 3, df.data_ptr())
    solver.synchronize()
    assert np.array_equal(df.cpu().numpy().view(np.uint64), ref.view(np.uint64))
    with rsdsfm.Solver(0, arith="fused") as sf:
        assert np.array_equal(sf.deep_flow(a, b).view(np.uint64), ref.view(np.uint64))
    # a size change in between rebuilds the workspace; the first size gives the same bits again
    solver.deep_flow(a[:50, :70], b[:50, :70])
    assert np.array_equal(solver.deep_flow(a, b).view(np.uint64), ref.view(np.uint64))


def test_bad_arguments_are_rejected(rsdsfm, solver):
    lib, ctx = solver.lib, solver._ctx
    a = np.zeros((20, 30, 3), np.uint8)
    out = np.zeros((20, 30, 2))
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    INVALID = -1
    assert lib.rsdsfm_deep_flow(None, p(a), p(a), 20, 30, 3, None, p(out)) == INVALID
    assert lib.rsdsfm_deep_flow(ctx, None, p(a), 20, 30, 3, None, p(out)) == INVALID
    assert lib.rsdsfm_deep_flow(ctx, p(a), p(a), 20, 30, 3, None, None) == INVALID
    assert lib.rsdsfm_deep_flow(ctx, p(a), p(a), 20, 30, 2, None, p(out)) == INVALID
    assert lib.rsdsfm_deep_flow(ctx, p(a), p(a), 1, 30, 3, None, p(out)) == INVALID
    assert lib.rsdsfm_deep_flow_dev(ctx, None, None, 20, 30, 3, None, None) == INVALID
    for bad in (dict(fixed_point_iterations=0), dict(sor_iterations=0), dict(downscale=1.0), dict(downscale=0.0), dict(omega=2.0), dict(omega=0.0)):
        prm = rsdsfm._flow_params(bad)
        assert lib.rsdsfm_deep_flow(ctx, p(a), p(a), 20, 30, 3, C.byref(prm), p(out)) == INVALID
        with pytest.raises(rsdsfm.RsdsfmError):
            solver.deep_flow(a, a, bad)


@pytest.mark.parametrize("rows,cols,K", [(480, 640, "galaxy_vga"), (720, 1280, "hd720")])
def test_accuracy_on_rendered_pairs(rsdsfm, solver, rows, cols, K):
    """mean end-point error <= 0.25 px and 95th percentile <= 1 px over the valid mask, motion scaled to a maximum flow of 5 px (the
    spec on a 240x320 render of the same scene: mean 0.033 px, 95th percentile 0.076 px)"""
    K = rsdsfm.synth.INTRINSICS[K]
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, 0.8)
    a, b, truth, mask = rsdsfm.synth.render_pair(rows, cols, K, v, w, k, 0.8, seed=rows)
    epe = np.sqrt(((solver.deep_flow(a, b) - truth) ** 2).sum(-1))[mask]
    print("%dx%d EPE mean %.4f p95 %.4f max %.3f" % (cols, rows, epe.mean(), np.percentile(epe, 95), epe.max()))
    assert epe.mean() <= 0.25 and np.percentile(epe, 95) <= 1.0


def test_end_to_end_flow_into_the_solve(rsdsfm, solver):
    """the device flow goes straight into solve_frame_dev (no host copy); the velocities against the truth: rotation error <= 10 % of
    |w|, direction of v within 5 degrees"""
    import torch

    rows, cols, gamma = 480, 640, 0.8
    K = rsdsfm.synth.INTRINSICS["galaxy_vga"]
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma)
    a, b, _, _ = rsdsfm.synth.render_pair(rows, cols, K, v, w, k, gamma, seed=3)
    dev = torch.device("cuda", 0)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    d_flow = torch.empty((rows, cols, 2), dtype=torch.float64, device=dev)
    d_map = torch.empty(rows * cols, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    solver.deep_flow_dev(da.data_ptr(), db.data_ptr(), rows, cols, 3, d_flow.data_ptr())
    r = solver.solve_frame_dev(d_flow.data_ptr(), rows, cols, K, gamma, d_map.data_ptr(), trials=50, tol=0.05, seed=1)
    solver.synchronize()
    w_err, v_err = rsdsfm.velocity_errors(r["w"], r["v"], w, v)
    print("inliers %d of %d, w error %.3g (|w| %.3g), v error %.3f deg" % (r["num_inliers"], r["n"], w_err, np.linalg.norm(w), np.degrees(v_err)))
    assert w_err <= 0.1 * np.linalg.norm(w)
    assert np.degrees(v_err) <= 5.0


def test_evaluate_real_run_computes_the_flow(rsdsfm, solver, tmp_path):
    """flow=None: frame2.png next to frame1.png, flow -> solve -> rectify on the device; the same bytes as a call that is given that
    flow as a .npy; optical_flow.png written"""
    rows, cols, gamma = 240, 320, 0.95
    K = tuple(x * 0.5 for x in rsdsfm.synth.INTRINSICS["galaxy_vga"])
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, target=4.0)
    a, b, _, _ = rsdsfm.synth.render_pair(rows, cols, K, v, w, k, gamma, seed=9)
    prefix = str(tmp_path) + "/"
    rsdsfm.formats.write_png(prefix + "frame1.png", a)
    rsdsfm.formats.write_png(prefix + "frame2.png", b)
    r1 = rsdsfm.evaluate.evaluate_real_run(solver, prefix, None, camera=K, gamma=gamma, out_dir=str(tmp_path / "out1"), trials=20)
    np.save(str(tmp_path / "flow.npy"), r1["flow"])
    r2 = rsdsfm.evaluate.evaluate_real_run(solver, prefix, str(tmp_path / "flow.npy"), camera=K, gamma=gamma, out_dir=str(tmp_path / "out2"), trials=20)
    assert np.array_equal(r1["flow"], solver.deep_flow(a, b))
    assert "flow" not in r2
    for key in ("depth_map", "depth_est", "gs_image", "backprojection", "coords", "R", "t", "v", "w"):
        assert np.array_equal(np.asarray(r1[key]), np.asarray(r2[key])), key
    assert r1["num_inliers"] == r2["num_inliers"] and r1["k"] == r2["k"]
    assert os.path.exists(str(tmp_path / "out1" / "optical_flow.png")) and not os.path.exists(str(tmp_path / "out2" / "optical_flow.png"))
    for name in ("MinimalDepth.png", "backprojection.png", "point_cloud.ply"):
        assert open(str(tmp_path / "out1" / name), "rb").read() == open(str(tmp_path / "out2" / name), "rb").read(), name
    # the frame2 array form gives the same flow
    r3 = rsdsfm.evaluate.evaluate_real_run(solver, a, None, camera=K, gamma=gamma, frame2=b, trials=20)
    assert np.array_equal(r3["flow"], r1["flow"]) and np.array_equal(r3["depth_map"], r1["depth_map"])
