"""GPU: the clip's last frame (include/rsdsfm_last_frame.h).  The advance (rsdsfm_advance_depth_dev) bit for bit against its definition
(tests/last_frame_spec_numpy.py) in both library builds, with guard bytes behind every plane; rsdsfm_last_frame_dev against its three
parts; argument errors; and the five clip calls with last_frame = 1, byte for byte against the public calls made one after another, and
against the last_frame = 0 calls wherever the flag must change nothing.  The clip is tests/test_gpu_stabilize.py's."""
import ctypes

import numpy as np
import pytest

import last_frame_cases as cases
import last_frame_spec_numpy as spec

pytestmark = pytest.mark.gpu

GUARD, TRIALS = 0xCD, 20
_want = {}


def _guarded(torch, dev, nbytes, fill):
    """nbytes device bytes of value `fill` with 16 guard bytes behind them: (the buffer, the guard)"""
    buf = torch.full((nbytes + 16,), GUARD, dtype=torch.uint8, device=dev)
    buf[:nbytes] = fill
    return buf[:nbytes], buf[nbytes:]


def _clean(*guards):
    for g in guards:
        assert (g.cpu().numpy() == GUARD).all()


def _spec(name, shape, k, gs):
    """the case and the spec's outputs, computed once and shared by both library builds"""
    key = (name, shape, k, gs)
    if key not in _want:
        d = cases.family(name, *shape, k)
        _want[key] = (d, spec.advance_depth(d["F"], d["Z"], d["v"], d["w"], d["k"], d["K"], d["gamma"], gs))
    return _want[key]


@pytest.fixture(scope="module", params=["reference", "fused"])
def solver(rsdsfm, request):
    with rsdsfm.Solver(0, arith=request.param) as s:
        yield s


# ---------------------------------------------------------------------------------------------------
# the advance
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_advance_is_the_spec_bit_for_bit(solver, shape):
    """every family, both shutter modes, k in {0, 0.3, -0.3}, with and without the plane and the counter; guard bytes behind the map, the
    plane and the counter; the same call twice gives the same bytes"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = shape
    npix = rows * cols
    for name in cases.FAMILIES:
        d0 = _spec(name, shape, cases.KS[0], False)[0]
        d_F, d_Z = torch.from_numpy(d0["F"]).to(dev), torch.from_numpy(np.ascontiguousarray(d0["Z"].T)).to(dev)
        out, g_out = _guarded(torch, dev, 8 * npix, 0x5A)
        plane, g_plane = _guarded(torch, dev, 8 * npix, 0x5A)
        count, g_count = _guarded(torch, dev, 8, 0x5A)
        torch.cuda.synchronize()
        for k in cases.KS:
            for gs in (False, True):
                d, (zmap, zplane, n) = _spec(name, shape, k, gs)
                for optional in (True, False):
                    for again in range(2 if (optional and k == 0.3 and not gs) else 1):
                        if not again:
                            out.fill_(0x5A), plane.fill_(0x5A), count.fill_(0x5A)
                        torch.cuda.synchronize()
                        solver.advance_depth_dev(d_F.data_ptr(), d_Z.data_ptr(), d["v"], d["w"], k, rows, cols, d["K"], d["gamma"], out.data_ptr(), gs,
                                                 plane.data_ptr() if optional else None, count.data_ptr() if optional else None)
                        solver.synchronize()
                        got = out.cpu().numpy().view(np.uint64).reshape(cols, rows).T
                        assert np.array_equal(got, zmap.view(np.uint64)), (name, shape, k, gs, optional, again)
                        if optional:
                            assert np.array_equal(plane.cpu().numpy().view(np.uint64).reshape(rows, cols), zplane), (name, shape, k, gs)
                            assert int(count.cpu().numpy().view(np.int64)[0]) == n, (name, shape, k, gs)
                        else:
                            assert (plane.cpu().numpy() == 0x5A).all() and (count.cpu().numpy() == 0x5A).all()
                if name == "empty":
                    assert n == 0 and not zmap.any()
        _clean(g_out, g_plane, g_count)
    assert _spec("model", shape, 0.0, False)[1][2] > 0 or npix < 16  # (a field of a few pixels leaves a 2 x 2 frame)


def test_host_convenience_and_launches(rsdsfm, solver):
    d, (zmap, zplane, n) = _spec("model", (17, 33), 0.3, False)
    got = solver.advance_depth(d["F"], d["Z"], d["v"], d["w"], d["k"], d["K"], d["gamma"], want_plane=True)
    assert np.array_equal(got[0].view(np.uint64), zmap.view(np.uint64)) and got[1] == n and np.array_equal(got[2], zplane)
    assert rsdsfm.advance_depth_launches(17, 33) == 3


@pytest.mark.parametrize("k", cases.KS)
def test_last_frame_call_equals_its_three_parts(rsdsfm, solver, k):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 65, 130
    d = _spec("model", (rows, cols), k, False)[0]
    d_F, d_Z = torch.from_numpy(d["F"]).to(dev), torch.from_numpy(np.ascontiguousarray(d["Z"].T)).to(dev)
    runs = []
    for one_call in (True, False):
        out, g0 = _guarded(torch, dev, 8 * rows * cols, 0x5A)
        R, g1 = _guarded(torch, dev, 8 * rows * 9, 0x5A)
        t, g2 = _guarded(torch, dev, 8 * rows * 3, 0x5A)
        count, g3 = _guarded(torch, dev, 8, 0x5A)
        torch.cuda.synchronize()
        if one_call:
            solver.last_frame_dev(d_F.data_ptr(), d_Z.data_ptr(), d["v"], d["w"], k, rows, cols, d["K"], d["gamma"], out.data_ptr(), R.data_ptr(), t.data_ptr(),
                                  d_count=count.data_ptr())
        else:
            solver.advance_depth_dev(d_F.data_ptr(), d_Z.data_ptr(), d["v"], d["w"], k, rows, cols, d["K"], d["gamma"], out.data_ptr(), d_count=count.data_ptr())
            v2, w2, k2 = rsdsfm.last_frame_motion(d["v"], d["w"], k)
            solver.pose_table_dev(v2, w2, k2, d["gamma"], rows, R.data_ptr(), t.data_ptr())
        solver.synchronize()
        _clean(g0, g1, g2, g3)
        runs.append([x.cpu().numpy().tobytes() for x in (out, R, t, count)])
    assert runs[0] == runs[1]
    assert np.frombuffer(runs[0][3], dtype=np.int64)[0] == _spec("model", (rows, cols), k, False)[1][2]
    if k == 0.0:  # the pair's own table, byte for byte
        R, t = (torch.zeros(rows * n, dtype=torch.float64, device=dev) for n in (9, 3))
        torch.cuda.synchronize()
        solver.pose_table_dev(d["v"], d["w"], 0.0, d["gamma"], rows, R.data_ptr(), t.data_ptr())
        solver.synchronize()
        assert R.cpu().numpy().tobytes() == runs[0][1] and t.cpu().numpy().tobytes() == runs[0][2]


def test_argument_errors_write_nothing(rsdsfm, solver):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 17, 33
    d = _spec("model", (rows, cols), 0.3, False)[0]
    d_F, d_Z = torch.from_numpy(d["F"]).to(dev), torch.from_numpy(np.ascontiguousarray(d["Z"].T)).to(dev)
    keep_F, keep_Z = d_F.cpu().numpy().tobytes(), d_Z.cpu().numpy().tobytes()
    bufs = {n: torch.full((size,), 0x5A, dtype=torch.uint8, device=dev) for n, size in (("out", 8 * rows * cols), ("plane", 8 * rows * cols + 16), ("count", 16),
                                                                                           ("R", 8 * rows * 9), ("t", 8 * rows * 3))}
    torch.cuda.synchronize()
    P = {n: b.data_ptr() for n, b in bufs.items()}
    nan, inf = float("nan"), float("inf")
    base = dict(F=d_F.data_ptr(), Z=d_Z.data_ptr(), v=d["v"], w=d["w"], k=0.3, rows=rows, cols=cols, K=d["K"], gamma=d["gamma"], out=P["out"], plane=P["plane"],
                count=P["count"])
    bad = [dict(rows=1), dict(cols=1), dict(rows=16385), dict(cols=16385), dict(F=0), dict(Z=0), dict(out=0), dict(out=base["F"]), dict(out=base["Z"]),
           dict(plane=base["F"]), dict(plane=P["out"]), dict(count=P["out"]), dict(count=P["plane"]), dict(count=base["Z"]), dict(plane=P["plane"] + 8),
           dict(count=P["count"] + 4), dict(v=[0.0, nan, 0.0]), dict(w=[inf, 0.0, 0.0]), dict(k=nan), dict(k=-inf), dict(gamma=nan), dict(gamma=inf), dict(gamma=0.0),
           dict(K=(0.0, 1.0, 0.0, 0.0)), dict(K=(1.0, nan, 0.0, 0.0))]

    def advance(a):
        solver.advance_depth_dev(a["F"], a["Z"], a["v"], a["w"], a["k"], a["rows"], a["cols"], a["K"], a["gamma"], a["out"], False, a["plane"], a["count"])

    def last(a, R=P["R"], t=P["t"]):
        solver.last_frame_dev(a["F"], a["Z"], a["v"], a["w"], a["k"], a["rows"], a["cols"], a["K"], a["gamma"], a["out"], R, t, False, a["plane"], a["count"])

    for change in bad:
        for call in (advance, last):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(dict(base, **change))
    for change in (dict(k=-1.0), dict(k=-2.5)):  # 1 + k <= 0: the motion of the second frame does not exist; the advance alone takes it
        with pytest.raises(rsdsfm.RsdsfmError):
            last(dict(base, **change))
    for R, t in ((0, P["t"]), (P["R"], 0), (P["R"], P["R"]), (P["out"], P["t"]), (P["R"], base["Z"]), (P["plane"], P["t"])):
        with pytest.raises(rsdsfm.RsdsfmError):
            last(base, R, t)
    lib, v3, f64, i32 = solver.lib, (ctypes.c_double * 3)(), ctypes.c_double, ctypes.c_int32
    for v, w in ((None, v3), (v3, None)):
        assert lib.rsdsfm_advance_depth_dev(solver._ctx, ctypes.c_void_p(base["F"]), ctypes.c_void_p(base["Z"]), v, w, f64(0.0), i32(rows), i32(cols), f64(1), f64(1),
                                            f64(0), f64(0), f64(0.8), i32(0), ctypes.c_void_p(P["out"]), None, None) == -1
    solver.synchronize()
    assert all((b.cpu().numpy() == 0x5A).all() for b in bufs.values())
    assert d_F.cpu().numpy().tobytes() == keep_F and d_Z.cpu().numpy().tobytes() == keep_Z


# ---------------------------------------------------------------------------------------------------
# the clip
# ---------------------------------------------------------------------------------------------------
LEVELS = ("stabilized", "filled", "cropped", "blended", "inpainted")
RADIUS, FEATHER, MIN_OVERLAP, MAX_EMPTY, MARGIN = 2, 8, 64, 200, 0
SOLVE_KEYS = ("scales", "A", "c", "broken", "A_s", "c_s", "M", "m", "valid")
LEVEL_KEYS = {"stabilized": ("images", "masks"), "filled": ("sources", "counts"), "cropped": ("crops", "crop_masks", "crop_sources", "crop_counts", "window"),
              "blended": ("blends", "blend_masks", "blend_sources", "gains", "blend_counts"), "inpainted": ("inpainted", "inpaint_sources", "inpaint_counts")}


@pytest.fixture(scope="module")
def clip(rsdsfm):
    """tests/test_gpu_stabilize.py's clip: 5 frames of 96 x 128, built here"""
    rows, cols, gamma = 96, 128, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    sc = 3.0 / np.abs(f0).max()
    frames, _, _ = rsdsfm.synth.render_sequence(5, rows, cols, K, v * sc, w * sc, k, gamma, seed=21, speeds=(1.0, 1.4, 0.8, 1.0))
    return frames, rows, cols, K, gamma, [3 + 5 * i for i in range(4)]


def _record(r, dm, R, t):
    sm = r["refine_summary"]
    return (r["n"], r["num_inliers"], r["best_trial"], r["flipped"], r["ransac_v"].tobytes(), r["ransac_w"].tobytes(), float(r["ransac_k"]), r["v"].tobytes(),
            r["w"].tobytes(), float(r["k"]), sm["num_iterations"], sm["num_successful_steps"], sm["termination"], sm["final_cost"], dm.cpu().numpy().tobytes(),
            R.cpu().numpy().tobytes(), t.cpu().numpy().tobytes())


def _clip_run(rsdsfm, torch, clip, level, last_frame=True, one_call=True, fused=False, batch=0, nframes=None):
    """the clip on a fresh context up to `level`: the level's ONE call, or (one_call=False) the solve and then nothing but per-frame public
    calls, in the order the drivers make them"""
    frames, rows, cols, K, gamma, seeds = clip
    if nframes:
        frames, seeds = frames[:nframes], seeds[:nframes - 1]
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    nr = n + (1 if last_frame else 0)
    depth = LEVELS.index(level)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)]
    img = lambda value: [torch.full_like(d_frames[0], value) for _ in range(nr)]
    byte = lambda value: [torch.full((rows, cols), value, dtype=torch.uint8, device=dev) for _ in range(nr)]
    f64 = lambda m: [torch.full((m,), np.nan, dtype=torch.float64, device=dev) for _ in range(nr)]
    d_stab, d_smask, d_source = img(77), byte(77), byte(GUARD)
    d_crop, d_cmask, d_csource = img(55), byte(55), byte(55)
    d_blend, d_bmask, d_bsource = img(33), byte(33), byte(33)
    d_inp, d_isrc = img(11), byte(11)
    dms, Rs, ts = f64(rows * cols), f64(rows * 9), f64(rows * 3)
    d_fused = f64(rows * cols) if fused else None
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a] if a is not None else None
    head = (ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs), ptrs(ts), ptrs(d_stab), ptrs(d_smask))
    kw = dict(d_fused=ptrs(d_fused), sigma=1.0, seeds=seeds, trials=TRIALS, last_frame=last_frame)
    kw_fill = dict(kw, d_sources=ptrs(d_source), fill_radius=RADIUS)
    kw_crop = dict(kw_fill, d_crop_sources=ptrs(d_csource), max_empty=MAX_EMPTY, margin=MARGIN)
    kw_blend = dict(kw_crop, blend_feather=FEATHER, blend_min_overlap=MIN_OVERLAP)
    with rsdsfm.Solver(0) as s:
        if batch:
            s.set_flow_batch(batch)
        if one_call:
            if level == "stabilized":
                r = s.stabilize_video_dev(*head, **kw)
            elif level == "filled":
                r = s.stabilize_video_filled_dev(*head, **kw_fill)
            elif level == "cropped":
                r = s.stabilize_video_cropped_dev(*head, ptrs(d_crop), ptrs(d_cmask), **kw_crop)
            elif level == "blended":
                r = s.stabilize_video_blended_dev(*head, ptrs(d_crop), ptrs(d_cmask), ptrs(d_blend), ptrs(d_bmask), ptrs(d_bsource), **kw_blend)
            else:
                r = s.stabilize_video_inpainted_dev(*head, ptrs(d_crop), ptrs(d_cmask), ptrs(d_blend), ptrs(d_bmask), ptrs(d_bsource), ptrs(d_inp), ptrs(d_isrc), **kw_blend)
            s.synchronize()
        else:
            r = s.solve_video_linked_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms[:n]), ptrs(d_flows), seeds=seeds, d_R=ptrs(Rs[:n]), d_t=ptrs(ts[:n]),
                                         trials=TRIALS, d_fused=ptrs(d_fused[:n]) if fused else None)
            scales = r["scales"]
            s.synchronize()
            torch.cuda.synchronize()  # (the clip call waits for the solve's lanes before it goes on)
            if last_frame:
                last = r["pairs"][n - 1]
                s.last_frame_dev(d_flows[n - 1].data_ptr(), dms[n - 1].data_ptr(), last["v"], last["w"], last["k"], rows, cols, K, gamma, dms[n].data_ptr(),
                                 Rs[n].data_ptr(), ts[n].data_ptr())
                if fused:
                    s.advance_depth_dev(d_flows[n - 1].data_ptr(), d_fused[n - 1].data_ptr(), last["v"], last["w"], last["k"], rows, cols, K, gamma, d_fused[n].data_ptr())
                scales = r["scales"] = np.append(scales, scales[n - 1])
            r["A_s"], r["c_s"] = rsdsfm.smooth_path(r["A"], r["c"], 1.0, 0, True)
            r["M"], r["m"] = rsdsfm.virtual_poses(r["A"], r["c"], r["A_s"], r["c_s"], scales, True, last_frame)
            neighbours = lambda p: list(zip(*rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], scales, p, RADIUS)))
            src = d_fused if fused else dms
            frame = lambda q: (d_frames[q].data_ptr(), 3, src[q].data_ptr(), Rs[q].data_ptr(), ts[q].data_ptr(), K, rows, cols)
            d_valid = torch.full((nr,), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            for p in range(nr):
                s.stabilize_frame_dev(*frame(p), r["M"][p], r["m"][p], d_stab[p].data_ptr(), d_smask[p].data_ptr(), d_valid=d_valid[p:].data_ptr())
            s.synchronize()
            r["valid"] = d_valid.cpu().numpy()
            if depth >= 1:
                d_cnt = torch.zeros((nr, 2 + 2 * RADIUS), dtype=torch.int64, device=dev)
                d_cnt[:, 1] = d_valid
                for p in range(nr):
                    d_source[p].copy_(d_smask[p])
                torch.cuda.synchronize()
                for p in range(nr):
                    for q, sid, nM, nm in neighbours(p):
                        s.stabilize_fill_frame_dev(*frame(int(q)), nM, nm, int(sid), d_stab[p].data_ptr(), d_smask[p].data_ptr(), d_source[p].data_ptr(),
                                                   d_cnt[p, int(sid):].data_ptr())
                s.synchronize()
                r["counts"] = d_cnt.cpu().numpy()
                r["counts"][:, 0] = rows * cols - r["counts"][:, 1:].sum(axis=1)
            if depth >= 2:
                window = r["window"] = s.crop_window_dev(ptrs(d_smask), rows, cols, MAX_EMPTY, MARGIN)
                d_cnt = torch.zeros((nr, 2 + 2 * RADIUS), dtype=torch.int64, device=dev)
                for a in d_crop + d_cmask + d_csource:
                    a.zero_()
                torch.cuda.synchronize()
                for p in range(nr if window[2] else 0):
                    for q, sid, nM, nm in [(p, 1, r["M"][p], r["m"][p])] + neighbours(p):
                        s.stabilize_window_frame_dev(*frame(int(q)), nM, nm, int(sid), window, d_crop[p].data_ptr(), d_cmask[p].data_ptr(), d_csource[p].data_ptr(),
                                                     d_cnt[p, int(sid):].data_ptr())
                s.synchronize()
                r["crop_counts"] = d_cnt.cpu().numpy()
                r["crop_counts"][:, 0] = rows * cols - r["crop_counts"][:, 1:].sum(axis=1)
            if depth >= 3:
                d_dist = torch.full((rows, cols), 99, dtype=torch.uint8, device=dev)
                d_layer, d_lmask = torch.zeros_like(d_frames[0]), torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
                d_sums = torch.zeros((nr, 2 * RADIUS, 8), dtype=torch.int64, device=dev)
                d_cnt = torch.zeros((nr, 2 * RADIUS, 2), dtype=torch.int64, device=dev)
                d_own = torch.zeros(nr, dtype=torch.int64, device=dev)
                for a in d_blend + d_bmask + d_bsource:
                    a.zero_()
                torch.cuda.synchronize()
                for p in range(nr if window[2] else 0):
                    s.stabilize_window_frame_dev(*frame(p), r["M"][p], r["m"][p], 1, window, d_blend[p].data_ptr(), d_bmask[p].data_ptr(), d_bsource[p].data_ptr(),
                                                 d_own[p:].data_ptr())
                    s.seam_distance_dev(d_bmask[p].data_ptr(), rows, cols, FEATHER, d_dist.data_ptr())
                    for q, sid, nM, nm in neighbours(p):
                        s.synchronize()
                        d_layer.zero_()
                        d_lmask.zero_()
                        torch.cuda.synchronize()
                        s.stabilize_window_frame_dev(*frame(int(q)), nM, nm, int(sid), window, d_layer.data_ptr(), d_lmask.data_ptr(), None, None)
                        s.seam_blend_layer_dev(d_layer.data_ptr(), d_lmask.data_ptr(), 3, rows, cols, d_dist.data_ptr(), int(sid), d_blend[p].data_ptr(),
                                               d_bmask[p].data_ptr(), d_bsource[p].data_ptr(), d_sums[p, int(sid) - 2].data_ptr(), d_cnt[p, int(sid) - 2].data_ptr(),
                                               feather=FEATHER, min_overlap=MIN_OVERLAP)
                s.synchronize()
                sums, per, own = d_sums.cpu().numpy().view(np.uint64), d_cnt.cpu().numpy(), d_own.cpu().numpy()
                r["gains"] = np.array([[rsdsfm.seam_gains(rec, 3, MIN_OVERLAP) for rec in f] for f in sums], dtype=np.uint32).reshape(nr, 2 * RADIUS, 3)
                r["blend_counts"] = np.concatenate([(rows * cols - own - per[:, :, 0].sum(axis=1))[:, None], (own - per[:, :, 1].sum(axis=1))[:, None],
                                                    per.reshape(nr, 4 * RADIUS)], axis=1)
            if depth >= 4:
                d_cnt = torch.full((nr,), -1, dtype=torch.int64, device=dev)
                for p in range(nr):
                    d_inp[p].copy_(d_blend[p])
                    d_isrc[p].copy_(d_bsource[p])
                torch.cuda.synchronize()
                for p in range(nr):
                    s.inpaint_frame_dev(d_inp[p].data_ptr(), d_bmask[p].data_ptr(), 3, rows, cols, d_isrc[p].data_ptr(), d_cnt[p:].data_ptr())
                s.synchronize()
                r["inpaint_counts"] = d_cnt.cpu().numpy()
        host = lambda a: [t.cpu().numpy() for t in a]
        r.update(records=[_record(x, dms[i], Rs[i], ts[i]) for i, x in enumerate(r["pairs"])], images=host(d_stab), masks=host(d_smask), sources=host(d_source),
                 crops=host(d_crop), crop_masks=host(d_cmask), crop_sources=host(d_csource), blends=host(d_blend), blend_masks=host(d_bmask),
                 blend_sources=host(d_bsource), inpainted=host(d_inp), inpaint_sources=host(d_isrc), maps=host(dms), Rs=host(Rs), ts=host(ts),
                 fused=host(d_fused) if fused else None)
    return r


def _same(got, want, keys):
    for k in keys:
        a, b = got[k], want[k]
        if isinstance(b, list):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), k
        elif isinstance(b, tuple):
            assert a == b, k
        else:
            assert np.asarray(a).shape == np.asarray(b).shape and np.asarray(a).tobytes() == np.asarray(b).tobytes(), k


_parts = {}


def _parts_of(rsdsfm, torch, clip, fused=False, batch=0):
    """the loop of public calls through every level, run once per configuration and left unchanged"""
    if (fused, batch) not in _parts:
        _parts[(fused, batch)] = _clip_run(rsdsfm, torch, clip, "inpainted", one_call=False, fused=fused, batch=batch)
    return _parts[(fused, batch)]


def _check_level(got, want, level, fused=False):
    """what the level's one call writes, against the loop of public calls: the solve, the last frame's map and tables, and every level up to it
    (a level that fills writes into the stabilised images and masks: those are compared at the level that was run)"""
    depth = LEVELS.index(level)
    assert got["records"] == want["records"] and len(got["records"]) == 4
    _same(got, want, SOLVE_KEYS + ("maps", "Rs", "ts") + (("fused",) if fused else ()))
    assert got["M"].shape == (5, 3, 3) and got["scales"].shape == (5,) and got["scales"][4] == got["scales"][3] and got["valid"].shape == (5,)
    if depth == 0:
        return  # (the parts' images went on to be filled: test_stabilised_clip... compares them)
    _same(got, want, [k for lv in LEVELS[:depth + 1] for k in LEVEL_KEYS[lv]])
    assert got["counts"].shape == (5, 2 + 2 * RADIUS)
    if depth >= 2:
        assert got["window"][2] >= 1 and got["crop_counts"].shape == (5, 2 + 2 * RADIUS)
    if depth >= 3:
        assert got["gains"].shape == (5, 2 * RADIUS, 3) and got["blend_counts"].shape == (5, 2 + 4 * RADIUS)
    if depth >= 4:
        assert got["inpaint_counts"].shape == (5,) and all(x.all() for x in got["inpaint_sources"])


def test_stabilised_clip_with_its_last_frame_equals_its_parts(rsdsfm, clip):
    """rsdsfm_stabilize_video_dev with last_frame = 1 against the public calls (the parts stop at this level: the levels above write into the
    stabilised images), and against the last_frame = 0 call: everything the solve writes, the smoothed path, and frames 0 .. np - 1"""
    import torch

    want = _clip_run(rsdsfm, torch, clip, "stabilized", one_call=False)
    got = _clip_run(rsdsfm, torch, clip, "stabilized")
    _check_level(got, want, "stabilized")
    _same(got, want, LEVEL_KEYS["stabilized"])
    off = _clip_run(rsdsfm, torch, clip, "stabilized", last_frame=False)
    assert got["records"] == off["records"]  # results, every pair's map and tables
    _same(got, off, ("A", "c", "broken", "A_s", "c_s", "links"))
    for name in ("scales", "M", "m", "valid"):
        assert off[name].shape[0] == 4 and np.asarray(got[name][:4]).tobytes() == np.asarray(off[name]).tobytes(), name
    assert len(got["images"]) == 5 and len(off["images"]) == 4
    for p in range(4):
        assert np.array_equal(got["images"][p], off["images"][p]) and np.array_equal(got["masks"][p], off["masks"][p]), p
    # the last frame: rendered, its mask a mask, its count the mask's
    assert set(np.unique(got["masks"][4])) <= {0, 1} and got["valid"][4] == int(got["masks"][4].sum()) > 0.5 * 96 * 128 and (got["images"][4] != 77).any()
    # k = 0 (no acceleration mode): the last frame's table is its pair's own, byte for byte
    assert got["pairs"][3]["k"] == 0.0 and np.array_equal(got["Rs"][4], got["Rs"][3]) and np.array_equal(got["ts"][4], got["ts"][3])
    # the advanced map holds at least 0.8 times as many depths as the pair's map (the spec on a model pair: 0.956, tests/test_last_frame_cpu.py)
    held, inliers = int((got["maps"][4] != 0).sum()), int(got["pairs"][3]["num_inliers"])
    print("last frame: %d depths from %d inliers (%.3f)" % (held, inliers, held / inliers))
    assert not np.isnan(got["maps"][4]).any() and held >= 0.8 * inliers


@pytest.mark.parametrize("level", LEVELS[1:])
def test_clip_levels_with_the_last_frame_equal_their_parts(rsdsfm, clip, level):
    import torch

    got = _clip_run(rsdsfm, torch, clip, level)
    _check_level(got, _parts_of(rsdsfm, torch, clip), level)
    # the last frame has only previous candidates, under the offsets' existing ids
    assert set(np.unique(got["sources"][4])) <= {0, 1, 2, 4}
    if level == "filled":
        off = _clip_run(rsdsfm, torch, clip, level, last_frame=False)
        assert got["records"] == off["records"]
        for q in range(4 - RADIUS):  # frames the last frame is no candidate of
            assert np.array_equal(got["images"][q], off["images"][q]) and np.array_equal(got["masks"][q], off["masks"][q]), q
            assert np.array_equal(got["sources"][q], off["sources"][q]) and np.array_equal(got["counts"][q], off["counts"][q]), q
        for q in range(4 - RADIUS, 4):  # frames it is: it gives what it gives under the id of its offset, and takes nothing from who came before it
            sid = 2 * (4 - q) + 1
            assert off["counts"][q][sid] == 0 and not (off["sources"][q] == sid).any()
            assert all(got["counts"][q][i] == off["counts"][q][i] for i in range(1, sid)), q  # own, and the candidates asked before it
        print("fill counts with the last frame", got["counts"].tolist(), "without", off["counts"].tolist())
        # (on this clip the frames before the last are full before the last frame is asked: it gives nothing, and takes from those before it)
        assert got["counts"][4][3] == got["counts"][4][5] == 0 and got["counts"][4][2] + got["counts"][4][4] > 0


def test_inpainted_clip_with_fused_maps(rsdsfm, clip):
    import torch

    got = _clip_run(rsdsfm, torch, clip, "inpainted", fused=True)
    _check_level(got, _parts_of(rsdsfm, torch, clip, fused=True), "inpainted", fused=True)
    assert not np.isnan(got["fused"][4]).any() and (got["fused"][4] != 0).sum() >= (got["maps"][4] != 0).sum()


def test_filled_clip_at_flow_batch_one(rsdsfm, clip):
    import torch

    got = _clip_run(rsdsfm, torch, clip, "filled", batch=1)
    want = _clip_run(rsdsfm, torch, clip, "filled", one_call=False, batch=1)
    _check_level(got, want, "filled")


def test_a_clip_of_two_frames_renders_two_frames(rsdsfm, clip):
    import torch

    got = _clip_run(rsdsfm, torch, clip, "stabilized", nframes=2)
    want = _clip_run(rsdsfm, torch, clip, "stabilized", one_call=False, nframes=2)
    assert got["records"] == want["records"] and len(got["records"]) == 1
    _same(got, want, SOLVE_KEYS + ("maps", "Rs", "ts", "images", "masks"))
    assert len(got["images"]) == 2 and got["valid"].shape == (2,) and got["M"].shape == (2, 3, 3)
    for p in range(2):
        assert got["valid"][p] == int(got["masks"][p].sum()) > 0 and set(np.unique(got["masks"][p])) <= {0, 1}


def test_wrappers_refuse_short_lists_and_bad_flags(rsdsfm, clip):
    import torch

    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    mk = lambda shape, dtype, n: [torch.zeros(shape, dtype=dtype, device=dev) for _ in range(n)]
    ptrs = lambda a: [t.data_ptr() for t in a]
    full = dict(dms=mk(rows * cols, torch.float64, 5), flows=mk((rows, cols, 2), torch.float64, 4), Rs=mk(rows * 9, torch.float64, 5), ts=mk(rows * 3, torch.float64, 5),
                stab=mk(frames[0].shape, torch.uint8, 5), smask=mk((rows, cols), torch.uint8, 5))
    extra = {k: mk(frames[0].shape if k in ("crop", "blend", "inp") else (rows, cols), torch.uint8, 5) for k in ("crop", "cmask", "blend", "bmask", "bsrc", "inp")}
    torch.cuda.synchronize()

    def call(s, name, short, **kw):
        a = {k: ptrs(v[:4] if k == short else v) for k, v in dict(full, **extra).items()}
        head = (ptrs(d_frames), rows, cols, 3, K, gamma, a["dms"], a["flows"], a["Rs"], a["ts"], a["stab"], a["smask"])
        tail = {"stabilize_video_dev": (), "stabilize_video_filled_dev": (), "stabilize_video_cropped_dev": (a["crop"], a["cmask"]),
                "stabilize_video_blended_dev": (a["crop"], a["cmask"], a["blend"], a["bmask"], a["bsrc"]),
                "stabilize_video_inpainted_dev": (a["crop"], a["cmask"], a["blend"], a["bmask"], a["bsrc"], a["inp"])}[name]
        return getattr(s, name)(*head, *tail, seeds=seeds, trials=TRIALS, sigma=1.0, **kw)

    with rsdsfm.Solver(0) as s:
        for name, shorts in (("stabilize_video_dev", ("dms", "Rs", "ts", "stab", "smask")), ("stabilize_video_filled_dev", ("stab", "smask")),
                             ("stabilize_video_cropped_dev", ("crop", "cmask")), ("stabilize_video_blended_dev", ("blend", "bmask", "bsrc")),
                             ("stabilize_video_inpainted_dev", ("inp", "dms"))):
            for short in shorts:
                with pytest.raises(rsdsfm.RsdsfmError, match="entries"):
                    call(s, name, short, last_frame=True)
        # the library itself: a value of the flag other than 0 and 1, and a last frame without a map of its own
        with pytest.raises(rsdsfm.RsdsfmError):
            call(s, "stabilize_video_dev", None, last_frame=2)
        a = ptrs(full["dms"])
        with pytest.raises(rsdsfm.RsdsfmError):
            s.stabilize_video_dev(ptrs(d_frames), rows, cols, 3, K, gamma, a[:4] + [0], ptrs(full["flows"]), ptrs(full["Rs"]), ptrs(full["ts"]), ptrs(full["stab"]),
                                  seeds=seeds, trials=TRIALS, last_frame=True)


def test_evaluate_real_sequence_with_the_last_frame(rsdsfm, clip, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, fill=2, inpaint=True, last_frame=True) writes F images per stage and one more row per CSV;
    without the flag the outputs are what they are without the argument; its ValueError"""
    frames, rows, cols, K, gamma, seeds = clip
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0, fill=2, inpaint=True)
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, out_dir=str(tmp_path / "last"), last_frame=True, **kw)
        off = ev(s, frames, out_dir=str(tmp_path / "off"), last_frame=False, **kw)
        plain = ev(s, frames, out_dir=str(tmp_path / "plain"), **kw)
        with pytest.raises(ValueError):
            ev(s, frames, camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, last_frame=True)
    assert set(out) == set(off) == set(plain)
    for k in plain:
        if k == "pairs":
            for o in (off, out):
                assert all(np.array_equal(a[f], b[f]) for a, b in zip(o[k], plain[k]) for f in ("depth_map", "flow", "gs_image", "R", "t"))
        elif k == "path_smoothed":
            assert all(np.array_equal(off[k][f], plain[k][f]) for f in plain[k])
            assert all(np.array_equal(out[k][f], plain[k][f]) for f in ("A_s", "c_s")) and all(np.array_equal(out[k][f][:4], plain[k][f]) for f in ("M", "m"))
            assert out[k]["M"].shape == (5, 3, 3)
        elif k == "links":
            assert off[k] == plain[k] == out[k]
        elif isinstance(plain[k], list):
            assert len(off[k]) == len(plain[k]) and all(np.array_equal(a, b) for a, b in zip(off[k], plain[k])), k
        else:
            assert np.array_equal(np.asarray(off[k]), np.asarray(plain[k])), k
    for k in ("scales", "A", "c", "broken"):
        assert np.array_equal(np.asarray(out[k]), np.asarray(plain[k])), k
    names = lambda d: sorted(x.name for x in (tmp_path / d).iterdir())
    assert names("off") == names("plain")
    assert sorted(set(names("last")) - set(names("plain"))) == ["stabilized_4.png", "stabilized_filled_4.png", "stabilized_inpainted_4.png"]
    for k in ("stabilized", "stab_masks", "stab_valid", "stab_filled", "stab_sources", "stab_inpainted", "inpaint_sources"):
        assert len(out[k]) == 5 and len(plain[k]) == 4, k
    assert out["fill_counts"].shape == (5, 6) and out["inpaint_counts"].shape == (5,)
    for p in range(4):  # the own rendering of the frames before the last is what it was
        assert np.array_equal(out["stabilized"][p], plain["stabilized"][p]) and out["stab_valid"][p] == plain["stab_valid"][p]
    assert set(np.unique(out["stab_sources"][4])) <= {0, 1, 2, 4} and out["inpaint_sources"][4].all()
    for stage in ("", "filled_", "inpainted_"):
        key = {"": "stabilized", "filled_": "stab_filled", "inpainted_": "stab_inpainted"}[stage]
        assert np.array_equal(rsdsfm.formats.read_png(str(tmp_path / "last" / ("stabilized_%s4.png" % stage))), out[key][4])
    for name in ("fill.csv", "inpaint.csv"):
        assert len((tmp_path / "last" / name).read_text().strip().split("\n")) == 1 + len((tmp_path / "plain" / name).read_text().strip().split("\n"))
    for name in ("poses.csv", "trajectory.csv", "path_smoothed.csv"):
        assert (tmp_path / "last" / name).read_text() == (tmp_path / "plain" / name).read_text()
