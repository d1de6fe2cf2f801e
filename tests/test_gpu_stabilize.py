"""GPU: the stabiliser's frame (rsdsfm_stabilize_frame_dev) bit for bit against its definition (tests/stabilize_spec_numpy.py) -- filled depth,
displacement plane, image, mask and the valid count --, the identity pose against the dense rectifier's bytes, the exact shift case, the
optional outputs and argument errors; and the clip call (rsdsfm_stabilize_video_dev) byte for byte against the public calls made one after
another.  Inputs as tests/test_gpu_rectify_dense.py's (tests/stabilize_cases.py) with the standard virtual pose."""
import numpy as np
import pytest

import rectify_dense_spec_numpy as dense
import stabilize_cases as cases
import stabilize_spec_numpy as spec
from test_gpu_video import _buffers, _record, _scaled_motion

pytestmark = pytest.mark.gpu

SHAPES = [((2, 2), dict(holes=0.4)),          # the whole pyramid in one cell; no whole word for the count
          ((5, 3), dict(holes=0.4)),          # smaller than any tile, odd both ways
          ((16, 64), dict(holes=0.4)),        # exactly one tile
          ((33, 68), dict(holes=0.4)),        # ragged tiles, the packed path
          ((33, 70), dict(holes=0.4)),        # the byte tail, in the warp and in the count
          ((150, 200), dict(holes=0.4, block=(30, 60, 40, 50), corner=(12, 17)))]  # several tiles; the push crosses several levels
BIG = SHAPES[-1]
CASES = [(shape, kw, ch, 0, 0, 0) for shape, kw in SHAPES for ch in (3, 1)]
CASES += [((33, 70), dict(holes=0.4), 3, it, 0, 0) for it in (1, 16)]
CASES += [((33, 70), dict(holes=0.4), 3, 0, mode, q5) for mode, q5 in ((0, 1), (1, 0))]
CASES += [((33, 70), dict(none_valid=True), 3, 0, 0, 0), ((33, 70), dict(holes=0.4, specials=True), 3, 0, 0, 0)]
CASES += [((300, 400), dict(holes=0.4, block=(60, 90, 120, 160), corner=(25, 31)), 3, 0, 0, 0)]  # 7 dense launches: the large levels
LAUNCHES = {(2, 2): 4, (5, 3): 4, (16, 64): 4, (33, 68): 4, (33, 70): 4, (150, 200): 5, (300, 400): 7}

_expected = {}


def _case(oracle, shape, kw, ch, it, mode, q5, M=cases.M_STD, m=cases.m_STD, tag="std"):
    """inputs and the spec's outputs, computed once per case and shared"""
    key = (shape, tuple(sorted(kw.items())), ch, it, mode, q5, tag)
    if key not in _expected:
        rows, cols = shape
        K, image, depth = cases.inputs(rows, cols, channels=ch, **kw)
        R, t = oracle.pose_table(cases.POSE["v"], cases.POSE["w"], cases.POSE["k"], cases.POSE["gamma"], rows)
        R = np.ascontiguousarray(R).reshape(rows, 9)
        _expected[key] = dict(K=K, image=image, depth=depth, R=R, t=t, M=M, m=m,
                              out=spec.stabilize_frame(image, depth, R, t, K, M, m, mode=mode, q5_mode=q5, iterations=it))
    return _expected[key]


def _run(torch, s, e, it, mode, q5, dense_call=False):
    """one call with every optional output; the output buffers start as 77 / NaN / -1"""
    dev = torch.device("cuda", 0)
    rows, cols = e["depth"].shape
    ch = 1 if e["image"].ndim == 2 else 3
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_img, d_dm, d_R, d_t = tt(e["image"]), tt(e["depth"].T), tt(e["R"]), tt(e["t"])
    out, mask = torch.full_like(d_img, 77), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
    filled = torch.full((cols, rows), np.nan, dtype=torch.float64, device=dev)
    disp = torch.full((rows, cols, 2), np.nan, dtype=torch.float32, device=dev)
    valid = torch.full((1,), -1, dtype=torch.int64, device=dev)
    if not np.isnan(e["out"]["disp"]).any():
        disp.fill_(12345.0)  # (NaN could not tell an unwritten pair from a NaN result)
    torch.cuda.synchronize()
    if dense_call:
        s.rectify_dense_frame_dev(d_img.data_ptr(), ch, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, out.data_ptr(), mask.data_ptr(),
                                  filled.data_ptr(), disp.data_ptr(), mode=mode, q5_mode=q5, iterations=it)
    else:
        s.stabilize_frame_dev(d_img.data_ptr(), ch, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, e["M"], e["m"], out.data_ptr(),
                              mask.data_ptr(), filled.data_ptr(), disp.data_ptr(), valid.data_ptr(), mode=mode, q5_mode=q5, iterations=it)
    s.synchronize()
    return dict(image=out.cpu().numpy(), mask=mask.cpu().numpy(), filled=filled.cpu().numpy().T, disp=disp.cpu().numpy(), valid=int(valid.cpu().numpy()[0]))


def _check(got, want, count=True):
    assert not np.isnan(got["filled"]).any()  # every double written
    assert np.array_equal(got["filled"].view(np.uint64), want["filled"].view(np.uint64))
    nan = np.isnan(want["disp"])
    assert np.array_equal(np.isnan(got["disp"]), nan)
    assert np.array_equal(got["disp"].view(np.uint32)[~nan], want["disp"].view(np.uint32)[~nan])
    assert np.array_equal(got["mask"], want["mask"])  # (1 or 0: no 77 left)
    assert np.array_equal(got["image"], want["image"])
    if count:
        assert got["valid"] == want["valid"] == int(want["mask"].sum())


@pytest.mark.parametrize("shape,kw,ch,it,mode,q5", CASES)
def test_stabilised_frame_equals_the_spec(oracle, rsdsfm, shape, kw, ch, it, mode, q5):
    import torch

    e = _case(oracle, shape, kw, ch, it, mode, q5)
    want = e["out"]
    if kw.get("none_valid"):
        assert not want["image"].any() and not want["mask"].any() and not want["filled"].any() and want["valid"] == 0
    elif shape[0] * shape[1] > 64 and mode == 0:
        assert want["mask"].any() and not want["mask"].all() and (want["image"] != e["image"]).any()  # something moved, something left the frame
    assert rsdsfm.stabilize_launches(*shape) == rsdsfm.rectify_dense_launches(*shape) == LAUNCHES[shape]
    assert rsdsfm.stabilize_launches(*shape, count=True) == LAUNCHES[shape] + 1
    with rsdsfm.Solver(0) as s:
        _check(_run(torch, s, e, it, mode, q5), want)


@pytest.mark.parametrize("shape,kw", [((33, 70), dict(holes=0.4)), BIG])
def test_identity_pose_writes_the_dense_rectifiers_bytes(oracle, rsdsfm, shape, kw):
    import torch

    e = _case(oracle, shape, kw, 3, 0, 0, 0, cases.M_ID, cases.m_ID, "id")
    with rsdsfm.Solver(0) as s:
        got, want = _run(torch, s, e, 0, 0, 0), _run(torch, s, e, 0, 0, 0, dense_call=True)
    for k in ("image", "mask", "filled", "disp"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["valid"] == int(want["mask"].sum()) > 0
    _check(got, e["out"])


def test_dense_and_stabilise_alternate_on_one_context(oracle, rsdsfm):
    """dense, stabilise, dense at two sizes on ONE context (one workspace, rebuilt only when the size changes): the spec's result every time"""
    import torch

    a = _case(oracle, (33, 70), dict(holes=0.4), 3, 0, 0, 0)
    b = _case(oracle, *BIG, 1, 0, 0, 0)
    want_dense = {id(e): dense.rectify_dense(e["image"], e["depth"], e["R"], e["t"], *e["K"]) for e in (a, b)}
    with rsdsfm.Solver(0) as s:
        for e in (a, b, a):
            _check(_run(torch, s, e, 0, 0, 0, dense_call=True), want_dense[id(e)], count=False)
            _check(_run(torch, s, e, 0, 0, 0), e["out"])
            _check(_run(torch, s, e, 0, 0, 0, dense_call=True), want_dense[id(e)], count=False)


def test_exact_shift_on_the_device(rsdsfm):
    import torch

    c = cases.shift_case()
    e = dict(c, out=dict(disp=np.zeros(1)))
    with rsdsfm.Solver(0) as s:
        got = _run(torch, s, e, 0, 0, 0)
        img, mask, valid = s.stabilize(c["image"], c["depth"], c["R"], c["t"], c["K"], c["M"], c["m"])  # the host convenience
    assert (got["disp"][..., 0] == 8.0).all() and (got["disp"][..., 1] == -4.0).all() and (got["filled"] == 4.0).all()
    assert np.array_equal(got["image"], c["want"]) and np.array_equal(got["mask"], c["mask"]) and got["valid"] == 640
    assert np.array_equal(img, c["want"]) and np.array_equal(mask, c["mask"]) and valid == 640


def test_outputs_are_optional_and_nothing_else_is_written(oracle, rsdsfm):
    """image only; image + count without a mask (the workspace's mask plane); image + mask: the same bytes every time"""
    import torch

    dev = torch.device("cuda", 0)
    e = _case(oracle, (33, 70), dict(holes=0.4), 3, 0, 0, 0)
    rows, cols = 33, 70
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_img, d_dm, d_R, d_t = tt(e["image"]), tt(e["depth"].T), tt(e["R"]), tt(e["t"])
    with rsdsfm.Solver(0) as s:
        for fill in (77, 0):
            for want_mask, want_count in ((False, False), (False, True), (True, False)):
                out = torch.full_like(d_img, fill)
                mask = torch.full((rows, cols), fill, dtype=torch.uint8, device=dev)
                valid = torch.full((3,), -1, dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                s.stabilize_frame_dev(d_img.data_ptr(), 3, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, e["M"], e["m"], out.data_ptr(),
                                      mask.data_ptr() if want_mask else None, d_valid=valid[1:].data_ptr() if want_count else None)
                s.synchronize()
                assert np.array_equal(out.cpu().numpy(), e["out"]["image"]), (fill, want_mask, want_count)
                assert np.array_equal(mask.cpu().numpy(), e["out"]["mask"]) if want_mask else (mask.cpu().numpy() == fill).all()
                assert valid.cpu().numpy().tolist() == [-1, e["out"]["valid"] if want_count else -1, -1]


def test_argument_errors(rsdsfm):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    img = torch.zeros((rows, cols, 3), dtype=torch.uint8, device=dev)
    out = torch.zeros_like(img)
    mask = torch.zeros((rows, cols + 4), dtype=torch.uint8, device=dev)
    valid = torch.zeros(2, dtype=torch.int64, device=dev)
    dm, R, t = torch.ones(rows * cols, dtype=torch.float64, device=dev), torch.zeros(rows * 9, dtype=torch.float64, device=dev), torch.zeros(rows * 3, dtype=torch.float64, device=dev)
    K = (50.0, 50.0, 32.0, 8.0)
    nanM, infm = np.eye(3), np.zeros(3)
    nanM[1, 2], infm[0] = np.nan, np.inf
    with rsdsfm.Solver(0) as s:
        call = lambda i=img.data_ptr(), ch=3, d=dm.data_ptr(), o=out.data_ptr(), r=rows, c=cols, M=np.eye(3), m=np.zeros(3), **kw: s.stabilize_frame_dev(
            i, ch, d, R.data_ptr(), t.data_ptr(), K, r, c, M, m, o, **kw)
        for bad in (dict(M=None), dict(m=None), dict(M=nanM), dict(m=infm),
                    dict(o=img.data_ptr()),  # aliased in and out
                    dict(o=0), dict(i=0), dict(d=0), dict(ch=2), dict(mode=2), dict(q5_mode=7), dict(iterations=17), dict(iterations=-1),
                    dict(r=1), dict(c=1), dict(c=16385), dict(o=out.data_ptr() + 1), dict(d_mask=mask.data_ptr() + 2), dict(d_valid=valid.data_ptr() + 4)):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        call(d_mask=mask.data_ptr(), d_valid=valid.data_ptr())  # the same arguments without a fault go through
        s.synchronize()


def test_destroy_releases_the_workspace(rsdsfm):
    """create / stabilise call with a count and no mask (pyramid, displacement plane and the mask plane: 10.7 MB at 1280 x 720) / destroy, 12
    times: the device's free memory does not go down by a leak's 129 MB.  Free memory is device-wide and other processes share the device, so a
    step larger than 40 MB is measured again, up to three times: a leak shows every time."""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 720, 1280
    img = torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
    out = torch.zeros_like(img)
    valid = torch.zeros(1, dtype=torch.int64, device=dev)
    dm, R, t = torch.ones(rows * cols, dtype=torch.float64, device=dev), torch.zeros(rows * 9, dtype=torch.float64, device=dev), torch.zeros(rows * 3, dtype=torch.float64, device=dev)
    K = (1000.0, 1000.0, 640.0, 360.0)

    def cycle():
        with rsdsfm.Solver(0) as s:
            for r, c in ((rows, cols), (100, 200), (rows, cols)):
                s.stabilize_frame_dev(img.data_ptr(), 1, dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, r, c, cases.M_STD, cases.m_STD, out.data_ptr(),
                                      d_valid=valid.data_ptr())
            s.synchronize()

    cycle()
    steps = []
    for _ in range(3):
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        for _ in range(12):
            cycle()
        steps.append((before - torch.cuda.mem_get_info()[0]) / 1e6)
        if steps[-1] < 40.0:
            break
    assert min(steps) < 40.0, steps


# ---------------------------------------------------------------------------------------------------
# the clip
# ---------------------------------------------------------------------------------------------------
TRIALS = 20


@pytest.fixture(scope="module")
def clip(rsdsfm):
    """tests/test_gpu_video_linked.py's clip"""
    rows, cols, gamma = 96, 128, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, 3.0)
    frames, _, _ = rsdsfm.synth.render_sequence(5, rows, cols, K, v, w, k, gamma, seed=21, speeds=(1.0, 1.4, 0.8, 1.0))
    return frames, rows, cols, K, gamma, [3 + 5 * i for i in range(4)]


def _clip_run(rsdsfm, torch, clip, batch, fused, translation, one_call):
    """the stabilised clip on a fresh context: rsdsfm_stabilize_video_dev, or the public calls one after another"""
    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)]
    d_fused = [torch.full((rows * cols,), np.nan, dtype=torch.float64, device=dev) for _ in range(n)] if fused else None
    d_stab = [torch.full_like(d_frames[0], 77) for _ in range(n)]
    d_smask = [torch.full((rows, cols), 77, dtype=torch.uint8, device=dev) for _ in range(n)]
    dms, Rs, ts = _buffers(torch, dev, n, rows, cols)
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a] if a is not None else None
    sigma = 1.0  # five frames: a window that has neighbours on both sides
    with rsdsfm.Solver(0) as s:
        if batch:
            s.set_flow_batch(batch)
        if one_call:
            r = s.stabilize_video_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs), ptrs(ts), ptrs(d_stab), ptrs(d_smask),
                                      d_fused=ptrs(d_fused), sigma=sigma, translation=translation, seeds=seeds, trials=TRIALS)
            s.synchronize()
        else:
            r = s.solve_video_linked_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), seeds=seeds, d_R=ptrs(Rs), d_t=ptrs(ts), trials=TRIALS,
                                         d_fused=ptrs(d_fused))
            r["A_s"], r["c_s"] = rsdsfm.smooth_path(r["A"], r["c"], sigma, 0, translation)
            r["M"], r["m"] = rsdsfm.virtual_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"] if translation else None, translation)
            d_valid = torch.full((n,), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            src = d_fused if fused else dms
            for p in range(n):
                s.stabilize_frame_dev(d_frames[p].data_ptr(), 3, src[p].data_ptr(), Rs[p].data_ptr(), ts[p].data_ptr(), K, rows, cols, r["M"][p], r["m"][p],
                                      d_stab[p].data_ptr(), d_smask[p].data_ptr(), d_valid=d_valid[p:].data_ptr())
            s.synchronize()
            r["valid"] = d_valid.cpu().numpy()
        r.update(records=[_record(x, dms[i], Rs[i], ts[i]) for i, x in enumerate(r["pairs"])], images=[t.cpu().numpy() for t in d_stab],
                 masks=[t.cpu().numpy() for t in d_smask], fused=[t.cpu().numpy() for t in d_fused] if fused else None)
    return r


@pytest.mark.parametrize("batch,fused,translation", [(1, False, True), (0, False, True), (0, True, True), (0, False, False)])
def test_stabilised_clip_equals_its_parts(rsdsfm, clip, batch, fused, translation):
    import torch

    want = _clip_run(rsdsfm, torch, clip, batch, fused, translation, one_call=False)
    got = _clip_run(rsdsfm, torch, clip, batch, fused, translation, one_call=True)
    assert got["records"] == want["records"]
    for name in ("scales", "A", "c", "broken", "A_s", "c_s", "M", "m", "valid"):
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name
    for p in range(4):
        assert np.array_equal(got["images"][p], want["images"][p]) and np.array_equal(got["masks"][p], want["masks"][p]), p
        assert got["valid"][p] == int(got["masks"][p].sum()) > 0.5 * 96 * 128
        assert (got["images"][p] != 77).any() and set(np.unique(got["masks"][p])) <= {0, 1}
        if fused:
            assert got["fused"][p].tobytes() == want["fused"][p].tobytes(), p
    assert np.abs(got["A_s"] - got["A"]).max() > 0  # the path moved
    if translation:
        assert np.abs(got["m"]).max() > 0
    else:
        assert not got["m"].any() and np.array_equal(got["c_s"], got["c"])


def test_the_clip_call_needs_every_table(rsdsfm, clip):
    import torch

    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.zeros((rows, cols, 2), dtype=torch.float64, device=dev) for _ in range(4)]
    d_stab = [torch.zeros_like(d_frames[0]) for _ in range(4)]
    dms, Rs, ts = _buffers(torch, dev, 4, rows, cols)
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a] if a is not None else None
    with rsdsfm.Solver(0) as s:
        base = dict(d_depth_maps=ptrs(dms), d_flows=ptrs(d_flows), d_R=ptrs(Rs), d_t=ptrs(ts))
        for missing in ("d_flows", "d_R", "d_t"):
            kw = dict(base, **{missing: None})
            with pytest.raises(rsdsfm.RsdsfmError, match="required"):
                s.stabilize_video_dev(ptrs(d_frames), rows, cols, 3, K, gamma, kw["d_depth_maps"], kw["d_flows"], kw["d_R"], kw["d_t"], ptrs(d_stab), trials=TRIALS)
        with pytest.raises(rsdsfm.RsdsfmError):
            s.stabilize_video_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs), ptrs(ts), ptrs(d_stab), sigma=0.0, trials=TRIALS)


def test_evaluate_real_sequence_with_stabilize(rsdsfm, clip, tmp_path):
    """evaluate_real_sequence(..., stabilize=True): the trajectory it returned before, smooth_path and virtual_poses on it, every frame as
    Solver.stabilize gives it, and the files; with stabilize=False the existing keys equal a call made without the new arguments"""
    frames, rows, cols, K, gamma, seeds = clip
    ev = rsdsfm.evaluate.evaluate_real_sequence
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, camera=K, gamma=gamma, out_dir=str(tmp_path / "stab"), trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
        plain = ev(s, frames, camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, trajectory=True)
        off = ev(s, frames, camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, trajectory=True, stabilize=False, smooth_sigma=2.0, smooth_translation=False)
        A_s, c_s = rsdsfm.smooth_path(out["A"], out["c"], 1.0)
        M, m = rsdsfm.virtual_poses(out["A"], out["c"], A_s, c_s, out["scales"])
        again = [s.stabilize(frames[p], out["pairs"][p]["depth_map"], out["pairs"][p]["R"], out["pairs"][p]["t"], K, M[p], m[p]) for p in range(4)]
    assert set(off) == set(plain) and set(out) == set(plain) | {"stabilized", "stab_masks", "stab_valid", "path_smoothed"}
    for name in ("scales", "A", "c", "broken"):
        assert np.array_equal(np.asarray(off[name]), np.asarray(plain[name])) and np.array_equal(np.asarray(out[name]), np.asarray(plain[name])), name
    for q in range(4):
        assert np.array_equal(off["points"][q].view(np.uint32), plain["points"][q].view(np.uint32))
        for k_ in ("depth_map", "gs_image", "flow", "v", "w"):
            assert np.array_equal(off["pairs"][q][k_], plain["pairs"][q][k_]) and np.array_equal(out["pairs"][q][k_], plain["pairs"][q][k_]), (q, k_)
    ps = out["path_smoothed"]
    for name, val in (("A_s", A_s), ("c_s", c_s), ("M", M), ("m", m)):
        assert np.array_equal(ps[name], val), name
    for p in range(4):
        img, mask, valid = again[p]
        assert np.array_equal(out["stabilized"][p], img) and np.array_equal(out["stab_masks"][p], mask) and out["stab_valid"][p] == valid == int(mask.sum())
        assert np.array_equal(rsdsfm.formats.read_png(str(tmp_path / "stab" / ("stabilized_%d.png" % p))), img)
    lines = (tmp_path / "stab" / "path_smoothed.csv").read_text().strip().split("\n")
    assert len(lines) == 1 + 5 and lines[0].startswith("frame,c_x") and len(lines[1].split(",")) == 13
    assert (tmp_path / "stab" / "trajectory.csv").exists()
