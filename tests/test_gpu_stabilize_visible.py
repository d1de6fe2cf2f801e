"""GPU: the occlusion test's frame call (rsdsfm_stabilize_visible_frame_dev) bit for bit against its definition
(tests/stabilize_visible_spec_numpy.py) in both library builds -- every case of tests/stabilize_visible_cases.py against the golden fixture
the CPU suite holds to the definition, 20 seeded random tiny frames, the constant-depth identity against rsdsfm_stabilize_window_frame_dev,
argument errors, alternation with the other calls on one context -- and the clip calls with rsdsfm_stabilize_fill_params.occlusion = 1 byte
for byte against the public calls made one after another.  The clip is tests/test_gpu_stabilize.py's, built here."""
import os

import numpy as np
import pytest

import rectify_dense_spec_numpy as dense
import stabilize_cases as stab_cases
import stabilize_visible_cases as cases

pytestmark = pytest.mark.gpu

GUARD = 0xCD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_stabilize_visible_v1.npz")


def _guarded(torch, dev, a):
    """a's bytes on the device with 16 guard bytes behind them: (the view of a's shape, the guard)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + 16,), GUARD, dtype=torch.uint8, device=dev)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[:a.size].view(*a.shape), buf[a.size:]


def _render(torch, s, case, visible=True, with_source=True, with_counts=True):
    """one visible call (or, visible=False, one rsdsfm_stabilize_window_frame_dev) on a case's planes; every plane has guard bytes behind it
    and the counters a guard on either side"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depth"].shape
    ch = 1 if case["image"].ndim == 2 else 3
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_n, d_dm, d_R, d_t = tt(case["image"]), tt(case["depth"].T), tt(case["R"]), tt(case["t"])
    (d_img, g_img), (d_mask, g_mask), (d_src, g_src) = (_guarded(torch, dev, case[k]) for k in ("image0", "mask0", "source0"))
    cnt = torch.full((4,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    head = (d_n.data_ptr(), ch, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), case["K"], rows, cols, case["M"], case["m"], cases.SID, case["window"])
    tail = (d_img.data_ptr(), d_mask.data_ptr(), d_src.data_ptr() if with_source else None, cnt[1:].data_ptr() if with_counts else None)
    kw = dict(mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    if visible:
        s.stabilize_visible_frame_dev(*head, *tail, tol_q16=case["tol_q16"], **kw)
    else:
        s.stabilize_window_frame_dev(*head, *tail, **kw)
    s.synchronize()
    for g in (g_img, g_mask, g_src):
        assert (g.cpu().numpy() == GUARD).all()
    c = cnt.cpu().numpy().tolist()
    assert c[0] == -1 and c[3] == -1 and (visible and with_counts or c[2] == -1)
    counts = (c[1], c[2]) if visible or not with_counts else (c[1], 0)  # the window call has one counter and rejects nothing
    return dict(image=d_img.cpu().numpy(), mask=d_mask.cpu().numpy(), source=d_src.cpu().numpy(), counts=counts)


def _same(got, want, name=""):
    for k in ("image", "mask", "source"):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert tuple(got["counts"]) == tuple(want["counts"]), (name, got["counts"], want["counts"])


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_every_case_equals_the_definition(oracle, rsdsfm, arith):
    """image, mask, source and [taken, rejected] of every case: the golden fixture, which tests/test_stabilize_visible_cpu.py holds to the spec"""
    import torch

    g = np.load(GOLDEN)
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in cases.all_cases(oracle.pose_table):
            n = case["name"] + "/"
            want = dict(image=g[n + "image"], mask=g[n + "mask"], source=g[n + "source"], counts=tuple(g[n + "counts"].tolist()))
            _same(_render(torch, s, case), want, case["name"])
            assert rsdsfm.stabilize_visible_launches(*case["depth"].shape) == rsdsfm.stabilize_window_launches(*case["depth"].shape)


def test_the_host_convenience_and_optional_outputs(oracle, rsdsfm):
    import torch

    case = cases.fold_case(37, 67, 3, -1, mask0=cases.pattern_mask(37, 67))
    want = cases.run_spec(case)
    with rsdsfm.Solver(0) as s:
        img, mask, source, taken, rejected = s.stabilize_visible(case["image"], case["depth"], case["R"], case["t"], case["K"], case["M"], case["m"], cases.SID,
                                                                 image=case["image0"], mask=case["mask0"], source=case["source0"])
        _same(dict(image=img, mask=mask, source=source, counts=(taken, rejected)), want)
        for with_source, with_counts in ((False, False), (False, True), (True, False)):
            got = _render(torch, s, case, with_source=with_source, with_counts=with_counts)
            assert np.array_equal(got["image"], want["image"]) and np.array_equal(got["mask"], want["mask"])
            assert np.array_equal(got["source"], want["source"] if with_source else case["source0"])
            assert got["counts"] == (want["counts"] if with_counts else (-1, -1))


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_constant_depth_is_the_window_call(rsdsfm, arith):
    """one surface cannot hide itself: on a constant depth the bytes are rsdsfm_stabilize_window_frame_dev's on the same inputs and nothing is
    rejected"""
    import torch

    z = stab_cases.shift_case()
    rng = np.random.default_rng(3)
    with rsdsfm.Solver(0, arith=arith) as s:
        for M, m in ((np.eye(3), z["m"]), (np.eye(3), np.array([-0.3, 0.2, 0.5])), (stab_cases.M_STD, stab_cases.m_STD)):
            for window in ((0, 0, 24, 40), (4, 14, 12, 20)):
                case = cases._case("constant", z["image"], z["depth"], z["R"], z["t"], z["K"], M, m, window, mask0=(rng.random((24, 40)) < 0.3).astype(np.uint8))
                got, plain = _render(torch, s, case), _render(torch, s, case, visible=False)
                assert got["counts"] == (plain["counts"][0], 0) and got["counts"][0] > 0
                _same(got, dict(plain, counts=got["counts"]))


def test_random_tiny_frames(rsdsfm):
    """20 seeded draws: rows, cols in 2 .. 70, a smooth depth plus a box, a small pose, a pre-set mask"""
    import torch

    seen = [0, 0]
    with rsdsfm.Solver(0) as s:
        for seed in range(20):
            case = cases.random_case(seed)
            want = cases.run_spec(case)
            _same(_render(torch, s, case), want, case["name"])
            seen = [seen[0] + want["counts"][0], seen[1] + want["counts"][1]]
    assert seen[0] > 1000 and seen[1] > 100  # both outcomes are exercised


def test_argument_errors(rsdsfm):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    img = torch.zeros((rows, cols, 3), dtype=torch.uint8, device=dev)
    out = torch.zeros_like(img)
    mask, source = torch.zeros((rows, cols + 4), dtype=torch.uint8, device=dev), torch.zeros((rows, cols + 4), dtype=torch.uint8, device=dev)
    counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
    dm, t = torch.ones(rows * cols, dtype=torch.float64, device=dev), torch.zeros(rows * 3, dtype=torch.float64, device=dev)
    R = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 9).repeat(rows, 1).contiguous()
    K = (50.0, 50.0, 32.0, 8.0)
    nanM = np.eye(3)
    nanM[1, 2] = np.nan
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        call = lambda i=img.data_ptr(), ch=3, d=dm.data_ptr(), o=out.data_ptr(), r=rows, c=cols, M=np.eye(3), m=np.zeros(3), sid=2, w=(2, 8, 8, 32), k=mask.data_ptr(), **kw: \
            s.stabilize_visible_frame_dev(i, ch, d, R.data_ptr(), t.data_ptr(), K, r, c, M, m, sid, w, o, k, **kw)
        for bad in (dict(tol_q16=-1), dict(tol_q16=65537), dict(d_counts2=counts.data_ptr() + 4), dict(w=None), dict(w=(0, 0, 0, 32)), dict(w=(9, 0, 8, 32)),
                    dict(w=(0, 33, 8, 32)), dict(M=None), dict(M=nanM), dict(o=img.data_ptr()), dict(d_source=mask.data_ptr()), dict(o=0), dict(k=0), dict(ch=2),
                    dict(mode=2), dict(iterations=17), dict(r=1), dict(sid=0), dict(sid=256), dict(o=out.data_ptr() + 1)):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        call(sid=255, w=(15, 63, 1, 1), d_source=source.data_ptr(), d_counts2=counts[1:].data_ptr(), tol_q16=65536)  # the same arguments without a fault go through
        call(sid=1, tol_q16=1)
        s.synchronize()
    assert counts.cpu().numpy().tolist() == [-1, rows * cols, 0, -1]  # constant depth, identity poses: every pixel of the empty mask is taken


def test_clip_params_are_refused(rsdsfm):
    """occlusion = 2 and a tolerance out of range in rsdsfm_stabilize_fill_params: refused by every clip call before anything runs"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    frames = [torch.zeros((rows, cols, 3), dtype=torch.uint8, device=dev) for _ in range(3)]
    plane = lambda: [torch.zeros((rows, cols), dtype=torch.uint8, device=dev) for _ in range(2)]
    image = lambda: [torch.zeros((rows, cols, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    f64 = lambda *shape: [torch.zeros(shape, dtype=torch.float64, device=dev) for _ in range(2)]
    ptrs = lambda a: [t.data_ptr() for t in a]
    keep = [frames, image(), plane(), image(), plane(), image(), plane(), plane(), f64(rows * cols), f64(rows, cols, 2), f64(rows, 9), f64(rows, 3)]
    stab, smask, crop_, cmask, blend, bmask, bsrc, dms, flows, Rs, ts = (ptrs(a) for a in keep[1:])
    head = (ptrs(frames), rows, cols, 3, (50.0, 50.0, 32.0, 8.0), 0.8, dms, flows, Rs, ts, stab, smask)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        for kw in (dict(occlusion=2), dict(occlusion=-1), dict(occlusion=True, occlusion_tol=1.5), dict(occlusion=True, occlusion_tol=0.0)):
            with pytest.raises(rsdsfm.RsdsfmError, match="occlusion"):
                s.stabilize_video_filled_dev(*head, fill_radius=1, **kw)
            with pytest.raises(rsdsfm.RsdsfmError, match="occlusion"):
                s.stabilize_video_cropped_dev(*head, crop_, cmask, fill_radius=1, **kw)
            with pytest.raises(rsdsfm.RsdsfmError, match="occlusion"):
                s.stabilize_video_blended_dev(*head, crop_, cmask, blend, bmask, bsrc, fill_radius=1, **kw)


def test_window_visible_and_dense_calls_alternate_on_one_context(oracle, rsdsfm):
    """window call -> visible call -> dense call -> visible call at another size on ONE context (one workspace; the two planes come with the
    first visible call and again after the size change): each gives its own definition's bytes"""
    import torch

    dev = torch.device("cuda", 0)
    a, b = cases.fold_case(37, 67, 3, 1, mask0=cases.pattern_mask(37, 67)), cases.dense_case(oracle.pose_table, "holes", 33, 70, channels=1, holes=0.4)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    with rsdsfm.Solver(0) as s:
        _same(_render(torch, s, a, visible=False), cases.run_spec(a, visible=False))
        _same(_render(torch, s, a), cases.run_spec(a))
        d_img, d_dm, d_R, d_t = tt(a["image"]), tt(a["depth"].T), tt(a["R"]), tt(a["t"])
        out, d_mask = torch.full_like(d_img, 77), torch.full((37, 67), 77, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        s.rectify_dense_frame_dev(d_img.data_ptr(), 3, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), a["K"], 37, 67, out.data_ptr(), d_mask.data_ptr())
        s.synchronize()
        want = dense.rectify_dense(a["image"], a["depth"], a["R"], a["t"], *a["K"])
        assert np.array_equal(out.cpu().numpy(), want["image"]) and np.array_equal(d_mask.cpu().numpy(), want["mask"])
        _same(_render(torch, s, b), cases.run_spec(b))
        _same(_render(torch, s, b, visible=False), cases.run_spec(b, visible=False))
        _same(_render(torch, s, a), cases.run_spec(a))


# ---------------------------------------------------------------------------------------------------
# the clip
# ---------------------------------------------------------------------------------------------------
TRIALS = 20
RADIUS = 2
TOL = 0.25  # 16384 / 65536: not the default, so that the word is seen to arrive


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


def _clip_run(rsdsfm, torch, clip, one_call, occlusion=True, tol=TOL, feather=8):
    """the blended clip (which makes the cropped clip, which makes the filled clip) on a fresh context: rsdsfm_stabilize_video_blended_dev with
    occlusion = 1, or rsdsfm_stabilize_video_dev and the three loops of public calls with rsdsfm_stabilize_visible_frame_dev for every neighbour"""
    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    n, npix, q16 = len(frames) - 1, rows * cols, int(round(tol * 65536))
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)]
    planes = lambda value, like=None: [torch.full_like(d_frames[0], value) if like else torch.full((rows, cols), value, dtype=torch.uint8, device=dev) for _ in range(n)]
    d_stab, d_smask, d_source = planes(77, True), planes(77), planes(GUARD)
    d_crop, d_cmask, d_csource = planes(55, True), planes(55), planes(55)
    d_blend, d_bmask, d_bsource = planes(33, True), planes(33), planes(33)
    dms = [torch.zeros(rows * cols, dtype=torch.float64, device=dev) for _ in range(n)]
    Rs = [torch.zeros((rows, 9), dtype=torch.float64, device=dev) for _ in range(n)]
    ts = [torch.zeros((rows, 3), dtype=torch.float64, device=dev) for _ in range(n)]
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a]
    solve = dict(sigma=1.0, seeds=seeds, trials=TRIALS)
    head = (ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs), ptrs(ts), ptrs(d_stab), ptrs(d_smask))
    with rsdsfm.Solver(0) as s:
        if one_call:
            r = s.stabilize_video_blended_dev(*head, ptrs(d_crop), ptrs(d_cmask), ptrs(d_blend), ptrs(d_bmask), ptrs(d_bsource), blend_feather=feather,
                                              blend_min_overlap=64, d_crop_sources=ptrs(d_csource), max_empty=200, margin=0, d_sources=ptrs(d_source),
                                              fill_radius=RADIUS, occlusion=occlusion, occlusion_tol=tol if occlusion else None, **solve)
            s.synchronize()
        else:
            r = s.stabilize_video_dev(*head, **solve)
            s.synchronize()
            cand = [list(zip(*rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p, RADIUS))) for p in range(n)]
            full = (0, 0, rows, cols)

            def neighbour(q, sid, nM, nm, window, image, mask, source, counts2):
                s.stabilize_visible_frame_dev(d_frames[q].data_ptr(), 3, dms[q].data_ptr(), Rs[q].data_ptr(), ts[q].data_ptr(), K, rows, cols, nM, nm, int(sid), window,
                                              image.data_ptr(), mask.data_ptr(), None if source is None else source.data_ptr(),
                                              None if counts2 is None else counts2.data_ptr(), tol_q16=q16)

            def own(p, window, image, mask, source, count):
                s.stabilize_window_frame_dev(d_frames[p].data_ptr(), 3, dms[p].data_ptr(), Rs[p].data_ptr(), ts[p].data_ptr(), K, rows, cols, r["M"][p], r["m"][p], 1, window,
                                             image.data_ptr(), mask.data_ptr(), source.data_ptr(), count.data_ptr())

            # the filled clip: the mask copied to the source plane, every neighbour through the full-frame window
            d_f2 = torch.zeros((n, 2 + 2 * RADIUS, 2), dtype=torch.int64, device=dev)
            for p in range(n):
                d_source[p].copy_(d_smask[p])
            torch.cuda.synchronize()
            for p in range(n):
                for q, sid, nM, nm in cand[p]:
                    neighbour(q, sid, nM, nm, full, d_stab[p], d_smask[p], d_source[p], d_f2[p, int(sid)])
            s.synchronize()
            counts = d_f2.cpu().numpy()[:, :, 0]
            counts[:, 1] = r["valid"]
            counts[:, 0] = npix - counts[:, 1:].sum(axis=1)
            r["counts"] = counts
            # the cropped clip
            r["window"] = s.crop_window_dev(ptrs(d_smask), rows, cols, 200, 0)
            d_c2 = torch.zeros((n, 2 + 2 * RADIUS, 2), dtype=torch.int64, device=dev)
            for a in d_crop + d_cmask + d_csource + d_blend + d_bmask + d_bsource:
                a.zero_()
            torch.cuda.synchronize()
            for p in range(n if r["window"][2] else 0):
                own(p, r["window"], d_crop[p], d_cmask[p], d_csource[p], d_c2[p, 1])
                for q, sid, nM, nm in cand[p]:
                    neighbour(q, sid, nM, nm, r["window"], d_crop[p], d_cmask[p], d_csource[p], d_c2[p, int(sid)])
            s.synchronize()
            r["crop_counts"] = d_c2.cpu().numpy()[:, :, 0]
            r["crop_counts"][:, 0] = npix - r["crop_counts"][:, 1:].sum(axis=1)
            r["crop_rejected"] = d_c2.cpu().numpy()[:, 2:, 1]
            # the blended clip: every neighbour alone on a layer
            d_dist = torch.full((rows, cols), 99, dtype=torch.uint8, device=dev)
            d_layer, d_lmask = torch.zeros_like(d_frames[0]), torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
            d_sums = torch.zeros((n, 2 * RADIUS, 8), dtype=torch.int64, device=dev)
            d_cnt = torch.zeros((n, 2 * RADIUS, 2), dtype=torch.int64, device=dev)
            d_own = torch.zeros(n, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            for p in range(n if r["window"][2] else 0):
                own(p, r["window"], d_blend[p], d_bmask[p], d_bsource[p], d_own[p:])
                s.seam_distance_dev(d_bmask[p].data_ptr(), rows, cols, feather, d_dist.data_ptr())
                for q, sid, nM, nm in cand[p]:
                    s.synchronize()
                    d_layer.zero_()
                    d_lmask.zero_()
                    torch.cuda.synchronize()
                    neighbour(q, sid, nM, nm, r["window"], d_layer, d_lmask, None, None)
                    s.seam_blend_layer_dev(d_layer.data_ptr(), d_lmask.data_ptr(), 3, rows, cols, d_dist.data_ptr(), int(sid), d_blend[p].data_ptr(), d_bmask[p].data_ptr(),
                                           d_bsource[p].data_ptr(), d_sums[p, int(sid) - 2].data_ptr(), d_cnt[p, int(sid) - 2].data_ptr(), feather=feather, min_overlap=64)
            s.synchronize()
            sums, per, own_n = d_sums.cpu().numpy().view(np.uint64), d_cnt.cpu().numpy(), d_own.cpu().numpy()
            r["gains"] = np.array([[rsdsfm.seam_gains(rec, 3, 64) for rec in frame] for frame in sums], dtype=np.uint32).reshape(n, 2 * RADIUS, 3)
            r["blend_counts"] = np.concatenate([(npix - own_n - per[:, :, 0].sum(axis=1))[:, None], (own_n - per[:, :, 1].sum(axis=1))[:, None], per.reshape(n, 4 * RADIUS)],
                                               axis=1)
        host = lambda a: [t.cpu().numpy() for t in a]
        r.update(images=host(d_stab), masks=host(d_smask), sources=host(d_source), crops=host(d_crop), crop_masks=host(d_cmask), crop_sources=host(d_csource),
                 blends=host(d_blend), blend_masks=host(d_bmask), blend_sources=host(d_bsource))
    return r


PLANES = ("images", "masks", "sources", "crops", "crop_masks", "crop_sources", "blends", "blend_masks", "blend_sources")
ARRAYS = ("scales", "A", "c", "A_s", "c_s", "M", "m", "valid", "counts", "crop_counts", "gains", "blend_counts")


def test_clips_with_occlusion_equal_their_parts(rsdsfm, clip):
    """the filled, the cropped and the blended clip with occlusion = 1: every output byte for byte the public calls made one after another, with
    rsdsfm_stabilize_visible_frame_dev where the neighbours' fill and window calls stood"""
    import torch

    want = _clip_run(rsdsfm, torch, clip, one_call=False)
    got = _clip_run(rsdsfm, torch, clip, one_call=True)
    npix = 96 * 128
    assert got["window"] == want["window"] and got["window"][2] >= 1
    for name in ARRAYS:
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name
    for p in range(4):
        for k in PLANES:
            assert np.array_equal(got[k][p], want[k][p]), (k, p)
        for counts, sources in ((got["counts"][p], got["sources"][p]), (got["crop_counts"][p], got["crop_sources"][p])):
            assert counts.sum() == npix and np.bincount(sources.reshape(-1), minlength=2 + 2 * RADIUS).tolist() == counts.tolist()
    print("window", got["window"], "counts", got["counts"].tolist(), "crop counts", got["crop_counts"].tolist(), "crop rejected", want["crop_rejected"].tolist())


def test_clips_without_occlusion_are_what_they_were(rsdsfm, clip, monkeypatch):
    """occlusion = 0 through the wrapper (struct_bytes = sizeof, both words 0) against a zero-initialised struct with only the radius set, which
    is what a caller built before the words had names passes: the same bytes everywhere"""
    import torch

    got = _clip_run(rsdsfm, torch, clip, one_call=True, occlusion=False)

    def zeroed(radius, occlusion=False, occlusion_tol=None):
        assert not occlusion and occlusion_tol is None
        return rsdsfm.StabilizeFillParams(int(radius), 0, 0, 0)

    monkeypatch.setattr(rsdsfm, "_stabilize_fill_params", zeroed)
    want = _clip_run(rsdsfm, torch, clip, one_call=True, occlusion=False)
    for name in ARRAYS:
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name
    for p in range(4):
        for k in PLANES:
            assert np.array_equal(got[k][p], want[k][p]), (k, p)


def test_evaluate_real_sequence_with_occlusion(rsdsfm, clip):
    """evaluate_real_sequence(..., stabilize=True, fill=2, crop=True, blend=True, occlusion=True): the keys and shapes of the call without the
    flag, every filled frame as Solver.stabilize_visible gives it candidate after candidate, counts that add up; occlusion needs fill"""
    frames, rows, cols, K, gamma, seeds = clip
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0, fill=2, crop=True, crop_margin=0, crop_max_empty=200, blend=True)
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, occlusion=True, occlusion_tol=TOL, **kw)
        plain = ev(s, frames, **kw)
        ps = out["path_smoothed"]
        again = []
        for p in range(4):
            img, mask = out["stabilized"][p], out["stab_masks"][p]
            source, counts = mask.copy(), [0, int(mask.sum()), 0, 0, 0, 0]
            for n, sid, nM, nm in zip(*rsdsfm.neighbour_poses(out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], p, 2)):
                o = out["pairs"][int(n)]
                img, mask, source, counts[int(sid)], _ = s.stabilize_visible(frames[int(n)], o["depth_map"], o["R"], o["t"], K, nM, nm, int(sid), image=img, mask=mask,
                                                                             source=source, tol_q16=int(round(TOL * 65536)))
            counts[0] = rows * cols - sum(counts[1:])
            again.append((img, source, counts))
        for bad in (dict(fill=0, blend=False), dict(stabilize=False, fill=0, crop=False, blend=False)):
            with pytest.raises(ValueError):
                ev(s, frames, occlusion=True, **dict(kw, **bad))
    assert set(out) == set(plain)
    for name in ("scales", "A", "c", "broken", "stab_valid"):
        assert np.array_equal(np.asarray(out[name]), np.asarray(plain[name])), name
    for p in range(4):
        assert np.array_equal(out["stabilized"][p], plain["stabilized"][p])
        assert np.array_equal(out["stab_filled"][p], again[p][0]) and np.array_equal(out["stab_sources"][p], again[p][1])
        assert out["fill_counts"][p].tolist() == again[p][2]
        for key in ("fill_counts", "crop_counts", "blend_counts"):
            assert out[key].shape == plain[key].shape and out[key][p].sum() == rows * cols
        assert out["stab_cropped"][p].shape == out["stab_blended"][p].shape == frames[0].shape
