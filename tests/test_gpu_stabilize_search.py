"""GPU: the visible pre-image search's frame call (rsdsfm_stabilize_search_frame_dev) bit for bit against its definition
(tests/stabilize_search_spec_numpy.py) in both library builds -- every case of tests/stabilize_search_cases.py against the golden fixture the
CPU suite holds to the definition, 20 seeded random tiny frames, argument errors, alternation with the other calls on one context -- and the
clip calls with the context's knob (rsdsfm_set_occlusion_search) byte for byte against the public calls made one after another, and without
it against themselves."""
import os

import numpy as np
import pytest

import rectify_dense_spec_numpy as dense
import stabilize_search_cases as cases
import stabilize_visible_cases as vcases

pytestmark = pytest.mark.gpu

GUARD = 0xCD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_stabilize_search_v1.npz")


def _guarded(torch, dev, a):
    """a's bytes on the device with 16 guard bytes behind them: (the view of a's shape, the guard)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + 16,), GUARD, dtype=torch.uint8, device=dev)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[:a.size].view(*a.shape), buf[a.size:]


def _render(torch, s, case, how="search", with_source=True, with_counts=True):
    """one search call (how: "search"), one rsdsfm_stabilize_visible_frame_dev ("visible") or one rsdsfm_stabilize_window_frame_dev ("window")
    on a case's planes; every plane has guard bytes behind it and the counters a guard on either side"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depth"].shape
    ch = 1 if case["image"].ndim == 2 else 3
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_n, d_dm, d_R, d_t = tt(case["image"]), tt(case["depth"].T), tt(case["R"]), tt(case["t"])
    (d_img, g_img), (d_mask, g_mask), (d_src, g_src) = (_guarded(torch, dev, case[k]) for k in ("image0", "mask0", "source0"))
    nc = dict(search=3, visible=2, window=1)[how]
    cnt = torch.full((5,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    head = (d_n.data_ptr(), ch, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), case["K"], rows, cols, case["M"], case["m"], cases.SID, case["window"])
    tail = (d_img.data_ptr(), d_mask.data_ptr(), d_src.data_ptr() if with_source else None, cnt[1:].data_ptr() if with_counts else None)
    kw = dict(mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    if how == "window":
        s.stabilize_window_frame_dev(*head, *tail, **kw)
    else:
        (s.stabilize_search_frame_dev if how == "search" else s.stabilize_visible_frame_dev)(*head, *tail, tol_q16=case["tol_q16"], **kw)
    s.synchronize()
    for g in (g_img, g_mask, g_src):
        assert (g.cpu().numpy() == GUARD).all()
    c = cnt.cpu().numpy().tolist()
    assert c[0] == -1 and all(x == -1 for x in c[1 + (nc if with_counts else 0):])
    return dict(image=d_img.cpu().numpy(), mask=d_mask.cpu().numpy(), source=d_src.cpu().numpy(), counts=tuple(c[1:1 + nc]))


def _same(got, want, name=""):
    for k in ("image", "mask", "source"):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert tuple(got["counts"]) == tuple(want["counts"]), (name, got["counts"], want["counts"])


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_every_case_equals_the_definition(oracle, rsdsfm, arith):
    """image, mask, source and [taken, rejected, recovered] of every case, gray and BGR, from the cases' random in-out planes: the golden
    fixture, which tests/test_stabilize_search_cpu.py holds to the spec.  The tie case is among them"""
    import torch

    g = np.load(GOLDEN)
    seen = np.zeros(3, dtype=np.int64)
    with rsdsfm.Solver(0, arith=arith) as s:
        all_cases = cases.all_cases(oracle.pose_table)
        assert cases.TIE_CASE in [c["name"] for c in all_cases] and {c["image"].ndim for c in all_cases} == {2, 3}
        for case in all_cases:
            n = case["name"] + "/"
            want = dict(image=g[n + "image"], mask=g[n + "mask"], source=g[n + "source"], counts=tuple(g[n + "counts"].tolist()))
            _same(_render(torch, s, case), want, case["name"])
            assert rsdsfm.stabilize_search_launches(*case["depth"].shape) == rsdsfm.stabilize_window_launches(*case["depth"].shape)
            seen += np.array(want["counts"])
    assert (seen > 0).all()


def test_the_host_convenience_and_optional_outputs(oracle, rsdsfm):
    """Solver.stabilize_search, and the frame call with each of d_source and d_counts3 absent"""
    import torch

    case = cases.fold_case(37, 67, 3, -1, mask0=cases.pattern_mask(37, 67))
    want = cases.run_spec(case)
    assert want["counts"][1] > 0 and want["counts"][2] > 0
    with rsdsfm.Solver(0) as s:
        img, mask, source, taken, rejected, recovered = s.stabilize_search(case["image"], case["depth"], case["R"], case["t"], case["K"], case["M"], case["m"], cases.SID,
                                                                           image=case["image0"], mask=case["mask0"], source=case["source0"])
        _same(dict(image=img, mask=mask, source=source, counts=(taken, rejected, recovered)), want)
        for with_source, with_counts in ((False, False), (False, True), (True, False)):
            got = _render(torch, s, case, with_source=with_source, with_counts=with_counts)
            assert np.array_equal(got["image"], want["image"]) and np.array_equal(got["mask"], want["mask"])
            assert np.array_equal(got["source"], want["source"] if with_source else case["source0"])
            assert got["counts"] == (want["counts"] if with_counts else (-1, -1, -1))


def test_random_tiny_frames(rsdsfm):
    """20 seeded draws: rows, cols in 2 .. 70, a smooth depth plus a box, a small pose, a pre-set mask; all three outcomes occur"""
    import torch

    seen = np.zeros(3, dtype=np.int64)
    with rsdsfm.Solver(0) as s:
        for seed in range(20):
            case = cases.random_case(seed)
            want = cases.run_spec(case)
            _same(_render(torch, s, case), want, case["name"])
            seen += np.array(want["counts"])
    assert seen[0] > 1000 and seen[1] > 100 and seen[2] > 300


def test_argument_errors(rsdsfm):
    """the visible call's list, a misaligned d_counts3, the knob's values and the keyword without occlusion; after each the same call without the
    fault goes through"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    img = torch.zeros((rows, cols, 3), dtype=torch.uint8, device=dev)
    out = torch.zeros_like(img)
    mask, source = torch.zeros((rows, cols + 4), dtype=torch.uint8, device=dev), torch.zeros((rows, cols + 4), dtype=torch.uint8, device=dev)
    counts = torch.full((5,), -1, dtype=torch.int64, device=dev)
    dm, t = torch.ones(rows * cols, dtype=torch.float64, device=dev), torch.zeros(rows * 3, dtype=torch.float64, device=dev)
    R = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 9).repeat(rows, 1).contiguous()
    K = (50.0, 50.0, 32.0, 8.0)
    nanM = np.eye(3)
    nanM[1, 2] = np.nan
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        call = lambda i=img.data_ptr(), ch=3, d=dm.data_ptr(), o=out.data_ptr(), r=rows, c=cols, M=np.eye(3), m=np.zeros(3), sid=2, w=(2, 8, 8, 32), k=mask.data_ptr(), **kw: \
            s.stabilize_search_frame_dev(i, ch, d, R.data_ptr(), t.data_ptr(), K, r, c, M, m, sid, w, o, k, **kw)
        for bad in (dict(tol_q16=-1), dict(tol_q16=65537), dict(d_counts3=counts.data_ptr() + 4), dict(w=None), dict(w=(0, 0, 0, 32)), dict(w=(9, 0, 8, 32)),
                    dict(w=(0, 33, 8, 32)), dict(M=None), dict(M=nanM), dict(o=img.data_ptr()), dict(d_source=mask.data_ptr()), dict(o=0), dict(k=0), dict(ch=2),
                    dict(mode=2), dict(iterations=17), dict(r=1), dict(sid=0), dict(sid=256), dict(o=out.data_ptr() + 1)):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
            call()  # the same call without the fault goes through
        for on in (2, -1):
            with pytest.raises(rsdsfm.RsdsfmError):
                s.set_occlusion_search(on)
            s.set_occlusion_search(1)
            s.set_occlusion_search(0)
        mask.zero_()
        out.zero_()
        torch.cuda.synchronize()
        call(sid=255, w=(15, 63, 1, 1), d_source=source.data_ptr(), d_counts3=counts[1:].data_ptr(), tol_q16=65536)
        s.synchronize()
        assert counts.cpu().numpy().tolist() == [-1, rows * cols, 0, 0, -1]  # constant depth, identity poses: every pixel of the empty mask is taken
        call(sid=1, tol_q16=1)
        # the clip wrappers: occlusion_search=True without occlusion is refused before anything runs, and the same call with occlusion goes through
        frames = [torch.zeros((rows, cols, 3), dtype=torch.uint8, device=dev) for _ in range(3)]
        plane = lambda: [torch.zeros((rows, cols), dtype=torch.uint8, device=dev) for _ in range(2)]
        image = lambda: [torch.zeros((rows, cols, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
        f64 = lambda *shape: [torch.zeros(shape, dtype=torch.float64, device=dev) for _ in range(2)]
        ptrs = lambda a: [x.data_ptr() for x in a]
        keep = [image(), plane(), image(), plane(), image(), plane(), plane(), image(), f64(rows * cols), f64(rows, cols, 2), f64(rows, 9), f64(rows, 3)]
        stab, smask, crop_, cmask, blend, bmask, bsrc, inp, dms, flows, Rs, ts = (ptrs(a) for a in keep)
        head = (ptrs(frames), rows, cols, 3, K, 0.8, dms, flows, Rs, ts, stab, smask)
        torch.cuda.synchronize()
        for name, extra in (("stabilize_video_filled_dev", ()), ("stabilize_video_cropped_dev", (crop_, cmask)),
                            ("stabilize_video_blended_dev", (crop_, cmask, blend, bmask, bsrc)), ("stabilize_video_inpainted_dev", (crop_, cmask, blend, bmask, bsrc, inp))):
            with pytest.raises(rsdsfm.RsdsfmError, match="occlusion"):
                getattr(s, name)(*head, *extra, fill_radius=1, occlusion_search=True)
        s.set_occlusion_search(1)
        with pytest.raises(rsdsfm.RsdsfmError, match="occlusion"):
            s.stabilize_video_filled_dev(*head, fill_radius=1, occlusion=2, occlusion_search=True)  # the fill params' own check still comes first
        assert s._occlusion_search == 1  # the keyword put the knob back where it was
        s.set_occlusion_search(0)
        s.synchronize()


def test_window_visible_search_and_dense_calls_alternate_on_one_context(oracle, rsdsfm):
    """window -> visible -> search -> dense -> search at another size -> visible on ONE context (one workspace; the search's planes come with
    its first call and again after the size change): each gives its own definition's bytes"""
    import torch

    dev = torch.device("cuda", 0)
    a, b = cases.fold_case(37, 67, 3, 1, mask0=cases.pattern_mask(37, 67)), vcases.dense_case(oracle.pose_table, "holes", 33, 70, channels=1, holes=0.4)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    with rsdsfm.Solver(0) as s:
        _same(_render(torch, s, a, "window"), dict(vcases.run_spec(a, visible=False), counts=vcases.run_spec(a, visible=False)["counts"][:1]))
        _same(_render(torch, s, a, "visible"), vcases.run_spec(a))
        _same(_render(torch, s, a), cases.run_spec(a))
        d_img, d_dm, d_R, d_t = tt(a["image"]), tt(a["depth"].T), tt(a["R"]), tt(a["t"])
        out, d_mask = torch.full_like(d_img, 77), torch.full((37, 67), 77, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        s.rectify_dense_frame_dev(d_img.data_ptr(), 3, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), a["K"], 37, 67, out.data_ptr(), d_mask.data_ptr())
        s.synchronize()
        want = dense.rectify_dense(a["image"], a["depth"], a["R"], a["t"], *a["K"])
        assert np.array_equal(out.cpu().numpy(), want["image"]) and np.array_equal(d_mask.cpu().numpy(), want["mask"])
        _same(_render(torch, s, b), cases.run_spec(b))
        _same(_render(torch, s, b, "visible"), vcases.run_spec(b))
        _same(_render(torch, s, a), cases.run_spec(a))


# ---------------------------------------------------------------------------------------------------
# the clips
# ---------------------------------------------------------------------------------------------------
TRIALS = 20
RADIUS = 2
TOL = 0.25  # 16384 / 65536: not the default, so that the word is seen to arrive
FEATHER = 4


def plain_clip(rsdsfm, scale=4.0, speeds=(1.0, 1.3)):
    """3 frames of 16 x 64: tests/test_gpu_stabilize.py's clip at the smallest size, its motion scaled to 4 pixels so that the own frame leaves
    a few pixels to the neighbours"""
    rows, cols, gamma = 16, 64, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    sc = scale / np.abs(f0).max()
    frames, _, _ = rsdsfm.synth.render_sequence(3, rows, cols, K, v * sc, w * sc, k, gamma, seed=21, speeds=speeds)
    return frames, rows, cols, K, gamma, [3, 8], (1, 4, 14, 56)


def fold_clip(rsdsfm, at=(-2.0, 0.0, 0.4, 2.4), back=0.3, box=1.5, dy=(0.0, 3.0, -3.0, 1.5)):
    """4 frames of 24 x 40, the camera at the positions `at` along x and shaken by `dy` pixels along y: a smooth background that moves `back`
    pixels per unit and, in front of it, the fold scene's box (stabilize_visible_cases.box_of, where it stands in the middle of the clip) that
    moves `box` -- the parallax the solve turns into a near depth, the shake what the stabiliser takes out and the neighbours fill.  The
    defaults were chosen among a few such clips for what the public frame calls count on them: the last frame leaves 159 pixels to its
    neighbours, the fill rejects 103 and the crop 96 candidates' pixels, and 70 pixels are recovered on the blend's layers"""
    rows, cols, gamma = 24, 40, 0.8
    K = (vcases.FX, vcases.FX, cols / 2.0, rows / 2.0)
    r0, r1, c0, c1 = vcases.box_of(rows, cols)
    y0, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    frames = []
    for f in range(4):
        xb, xn, y = x - back * at[f], x - box * at[f], y0 - dy[f]
        back = 60.0 + 30.0 * np.sin(0.9 * xb + 0.3 * y) + 20.0 * np.cos(0.5 * y - 0.4 * xb)
        near = 200.0 + 40.0 * np.sin(1.3 * xn - 0.7 * y) * np.cos(0.6 * y)
        inside = (y >= r0) & (y < r1) & (xn >= c0) & (xn < c1)
        g = np.where(inside, near, back)
        frames.append(np.clip(np.rint(np.stack([g, 0.9 * g + 12.0, 1.1 * g - 12.0], axis=-1)), 0, 255).astype(np.uint8))
    return np.stack(frames), rows, cols, K, gamma, [3, 8, 13], (2, 3, 19, 31)


@pytest.fixture(scope="module", params=["plain-16x64", "fold-24x40"])
def clip(request, rsdsfm):
    return dict(name=request.param, data=(plain_clip if request.param.startswith("plain") else fold_clip)(rsdsfm), runs={})


PLANES = ("images", "masks", "sources", "crops", "crop_masks", "crop_sources", "blends", "blend_masks", "blend_sources", "inpainted", "inpaint_sources")
ARRAYS = ("scales", "A", "c", "A_s", "c_s", "M", "m", "valid", "counts", "crop_counts", "gains", "blend_counts", "inpaint_counts")


def _clip_run(rsdsfm, torch, clip, how, knob=None, occlusion=True):
    """the inpainted clip (which makes the blended clip, which makes the cropped clip, which makes the filled clip) on a fresh context, the
    knob set first (None: never touched).  how "one": rsdsfm_stabilize_video_inpainted_dev; "parts": rsdsfm_stabilize_video_dev and the loops
    of public calls with rsdsfm_stabilize_search_frame_dev for every neighbour; "four": the four clip calls one after another with the
    keyword occlusion_search=knob, each on the planes of its own stage (the last one's outputs are returned).  Runs are kept per clip"""
    key = (how, knob, occlusion)
    if key in clip["runs"]:
        return clip["runs"][key]
    frames, rows, cols, K, gamma, seeds, window_in = clip["data"]
    dev = torch.device("cuda", 0)
    n, npix, q16 = len(frames) - 1, rows * cols, int(round(TOL * 65536))
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)]
    planes = lambda value, like=None: [torch.full_like(d_frames[0], value) if like else torch.full((rows, cols), value, dtype=torch.uint8, device=dev) for _ in range(n)]
    d_stab, d_smask, d_source = planes(77, True), planes(77), planes(GUARD)
    d_crop, d_cmask, d_csource = planes(55, True), planes(55), planes(55)
    d_blend, d_bmask, d_bsource = planes(33, True), planes(33), planes(33)
    d_inp, d_isrc = planes(11, True), planes(11)
    dms = [torch.zeros(rows * cols, dtype=torch.float64, device=dev) for _ in range(n)]
    Rs = [torch.zeros((rows, 9), dtype=torch.float64, device=dev) for _ in range(n)]
    ts = [torch.zeros((rows, 3), dtype=torch.float64, device=dev) for _ in range(n)]
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a]
    solve = dict(sigma=1.0, seeds=seeds, trials=TRIALS)
    head = (ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs), ptrs(ts), ptrs(d_stab), ptrs(d_smask))
    occ = dict(fill_radius=RADIUS, occlusion=occlusion, occlusion_tol=TOL if occlusion else None)
    crop_kw = dict(d_crop_sources=ptrs(d_csource), window_in=window_in, d_sources=ptrs(d_source))
    blend_kw = dict(blend_feather=FEATHER, blend_min_overlap=64)
    with rsdsfm.Solver(0) as s:
        if knob is not None and how != "four":
            s.set_occlusion_search(knob)
        if how == "one":
            r = s.stabilize_video_inpainted_dev(*head, ptrs(d_crop), ptrs(d_cmask), ptrs(d_blend), ptrs(d_bmask), ptrs(d_bsource), ptrs(d_inp), ptrs(d_isrc), **blend_kw,
                                                **crop_kw, **occ, **solve)
            s.synchronize()
        elif how == "four":
            kw = dict(occ, occlusion_search=bool(knob), **solve)
            r = s.stabilize_video_filled_dev(*head, d_sources=ptrs(d_source), **kw)
            filled = dict(images=[t.cpu().numpy() for t in d_stab], masks=[t.cpu().numpy() for t in d_smask], sources=[t.cpu().numpy() for t in d_source],
                          counts=r["counts"])
            r = s.stabilize_video_cropped_dev(*head, ptrs(d_crop), ptrs(d_cmask), **crop_kw, **kw)
            r = s.stabilize_video_blended_dev(*head, ptrs(d_crop), ptrs(d_cmask), ptrs(d_blend), ptrs(d_bmask), ptrs(d_bsource), **blend_kw, **crop_kw, **kw)
            r = s.stabilize_video_inpainted_dev(*head, ptrs(d_crop), ptrs(d_cmask), ptrs(d_blend), ptrs(d_bmask), ptrs(d_bsource), ptrs(d_inp), ptrs(d_isrc), **blend_kw,
                                                **crop_kw, **kw)
            s.synchronize()
            r["filled_alone"] = filled
            assert getattr(s, "_occlusion_search", 0) == 0  # the keyword put the knob back
        else:
            r = s.stabilize_video_dev(*head, **solve)
            s.synchronize()
            cand = [list(zip(*rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p, RADIUS))) for p in range(n)]
            full = (0, 0, rows, cols)

            def neighbour(q, sid, nM, nm, window, image, mask, source, counts3):
                s.stabilize_search_frame_dev(d_frames[q].data_ptr(), 3, dms[q].data_ptr(), Rs[q].data_ptr(), ts[q].data_ptr(), K, rows, cols, nM, nm, int(sid), window,
                                             image.data_ptr(), mask.data_ptr(), None if source is None else source.data_ptr(),
                                             None if counts3 is None else counts3.data_ptr(), tol_q16=q16)

            def own(p, window, image, mask, source, count):
                s.stabilize_window_frame_dev(d_frames[p].data_ptr(), 3, dms[p].data_ptr(), Rs[p].data_ptr(), ts[p].data_ptr(), K, rows, cols, r["M"][p], r["m"][p], 1, window,
                                             image.data_ptr(), mask.data_ptr(), source.data_ptr(), count.data_ptr())

            # the filled clip: the mask copied to the source plane, every neighbour through the full-frame window
            d_f3 = torch.zeros((n, 2 + 2 * RADIUS, 3), dtype=torch.int64, device=dev)
            for p in range(n):
                d_source[p].copy_(d_smask[p])
            torch.cuda.synchronize()
            for p in range(n):
                for q, sid, nM, nm in cand[p]:
                    neighbour(q, sid, nM, nm, full, d_stab[p], d_smask[p], d_source[p], d_f3[p, int(sid)])
            s.synchronize()
            f3 = d_f3.cpu().numpy()
            counts = f3[:, :, 0] + f3[:, :, 2]  # a recovered pixel counts under its offset
            counts[:, 1] = r["valid"]
            counts[:, 0] = npix - counts[:, 1:].sum(axis=1)
            r["counts"] = counts
            # the cropped clip
            r["window"] = tuple(window_in)
            d_c3 = torch.zeros((n, 2 + 2 * RADIUS, 3), dtype=torch.int64, device=dev)
            for a in d_crop + d_cmask + d_csource + d_blend + d_bmask + d_bsource:
                a.zero_()
            torch.cuda.synchronize()
            for p in range(n):
                own(p, r["window"], d_crop[p], d_cmask[p], d_csource[p], d_c3[p, 1])
                for q, sid, nM, nm in cand[p]:
                    neighbour(q, sid, nM, nm, r["window"], d_crop[p], d_cmask[p], d_csource[p], d_c3[p, int(sid)])
            s.synchronize()
            c3 = d_c3.cpu().numpy()
            r["crop_counts"] = c3[:, :, 0] + c3[:, :, 2]
            r["crop_counts"][:, 0] = npix - r["crop_counts"][:, 1:].sum(axis=1)
            r["recovered"] = int(f3[:, 2:, 2].sum()), int(c3[:, 2:, 2].sum())
            r["rejected"] = int(f3[:, 2:, 1].sum()), int(c3[:, 2:, 1].sum())
            # the blended clip: every neighbour alone on a layer
            d_dist = torch.full((rows, cols), 99, dtype=torch.uint8, device=dev)
            d_layer, d_lmask = torch.zeros_like(d_frames[0]), torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
            d_sums = torch.zeros((n, 2 * RADIUS, 8), dtype=torch.int64, device=dev)
            d_cnt = torch.zeros((n, 2 * RADIUS, 2), dtype=torch.int64, device=dev)
            d_own = torch.zeros(n, dtype=torch.int64, device=dev)
            d_l3 = torch.zeros((n, 2 + 2 * RADIUS, 3), dtype=torch.int64, device=dev)  # (the clip call passes no counters here: the bytes do not depend on them)
            torch.cuda.synchronize()
            for p in range(n):
                own(p, r["window"], d_blend[p], d_bmask[p], d_bsource[p], d_own[p:])
                s.seam_distance_dev(d_bmask[p].data_ptr(), rows, cols, FEATHER, d_dist.data_ptr())
                for q, sid, nM, nm in cand[p]:
                    s.synchronize()
                    d_layer.zero_()
                    d_lmask.zero_()
                    torch.cuda.synchronize()
                    neighbour(q, sid, nM, nm, r["window"], d_layer, d_lmask, None, d_l3[p, int(sid)])
                    s.seam_blend_layer_dev(d_layer.data_ptr(), d_lmask.data_ptr(), 3, rows, cols, d_dist.data_ptr(), int(sid), d_blend[p].data_ptr(), d_bmask[p].data_ptr(),
                                           d_bsource[p].data_ptr(), d_sums[p, int(sid) - 2].data_ptr(), d_cnt[p, int(sid) - 2].data_ptr(), feather=FEATHER, min_overlap=64)
            s.synchronize()
            sums, per, own_n, l3 = d_sums.cpu().numpy().view(np.uint64), d_cnt.cpu().numpy(), d_own.cpu().numpy(), d_l3.cpu().numpy()
            r["recovered"] += (int(l3[:, 2:, 2].sum()),)  # (filled, cropped, on the blend's layers)
            r["rejected"] += (int(l3[:, 2:, 1].sum()),)
            r["gains"] = np.array([[rsdsfm.seam_gains(rec, 3, 64) for rec in frame] for frame in sums], dtype=np.uint32).reshape(n, 2 * RADIUS, 3)
            r["blend_counts"] = np.concatenate([(npix - own_n - per[:, :, 0].sum(axis=1))[:, None], (own_n - per[:, :, 1].sum(axis=1))[:, None], per.reshape(n, 4 * RADIUS)],
                                               axis=1)
            # the inpainted clip: the blended frame and its sources copied, then invented where the blend's mask is empty
            d_icnt = torch.full((n,), -1, dtype=torch.int64, device=dev)
            for p in range(n):
                d_inp[p].copy_(d_blend[p])
                d_isrc[p].copy_(d_bsource[p])
            torch.cuda.synchronize()
            for p in range(n):
                s.inpaint_frame_dev(d_inp[p].data_ptr(), d_bmask[p].data_ptr(), 3, rows, cols, d_isrc[p].data_ptr(), d_icnt[p:].data_ptr())
            s.synchronize()
            r["inpaint_counts"] = d_icnt.cpu().numpy()
        host = lambda a: [t.cpu().numpy() for t in a]
        r.update(images=host(d_stab), masks=host(d_smask), sources=host(d_source), crops=host(d_crop), crop_masks=host(d_cmask), crop_sources=host(d_csource),
                 blends=host(d_blend), blend_masks=host(d_bmask), blend_sources=host(d_bsource), inpainted=host(d_inp), inpaint_sources=host(d_isrc))
    clip["runs"][key] = r
    return r


def _equal_runs(got, want, n, arrays=ARRAYS, planes=PLANES):
    for name in arrays:
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name
    for p in range(n):
        for k in planes:
            assert np.array_equal(got[k][p], want[k][p]), (k, p)


def test_clips_with_the_knob_equal_their_parts(rsdsfm, clip):
    """the knob at 1 and occlusion = 1: every output of the filled, cropped, blended and inpainted clip byte for byte the public calls made one
    after another, with rsdsfm_stabilize_search_frame_dev where the neighbours' calls stood; recovered pixels count under their offset"""
    import torch

    n, npix = len(clip["data"][0]) - 1, clip["data"][1] * clip["data"][2]
    want = _clip_run(rsdsfm, torch, clip, "parts")
    got = _clip_run(rsdsfm, torch, clip, "one", knob=1)
    assert tuple(got["window"]) == tuple(want["window"]) == tuple(clip["data"][6])
    _equal_runs(got, want, n)
    for p in range(n):
        for counts, sources in ((got["counts"][p], got["sources"][p]), (got["crop_counts"][p], got["crop_sources"][p])):
            assert counts.sum() == npix and np.bincount(sources.reshape(-1), minlength=2 + 2 * RADIUS).tolist() == counts.tolist()
    print(clip["name"], "counts", got["counts"].tolist(), "crop counts", got["crop_counts"].tolist(), "recovered (filled, cropped, blend layers)", want["recovered"],
          "rejected", want["rejected"])


def test_the_keyword_is_the_knob_for_each_of_the_four_calls(rsdsfm, clip):
    """stabilize_video_{filled, cropped, blended, inpainted}_dev(..., occlusion_search=True), one after another on one context: each its
    stage's bytes of the run with the knob set, and the knob back at 0 after each"""
    import torch

    n = len(clip["data"][0]) - 1
    want = _clip_run(rsdsfm, torch, clip, "one", knob=1)
    got = _clip_run(rsdsfm, torch, clip, "four", knob=1)
    _equal_runs(got, want, n)
    _equal_runs(got["filled_alone"], want, n, arrays=("counts",), planes=("images", "masks", "sources"))


def test_the_knob_without_occlusion_changes_nothing(rsdsfm, clip):
    """the knob at 1 and occlusion = 0: the clip call's bytes with the knob off"""
    import torch

    n = len(clip["data"][0]) - 1
    _equal_runs(_clip_run(rsdsfm, torch, clip, "one", knob=1, occlusion=False), _clip_run(rsdsfm, torch, clip, "one", knob=0, occlusion=False), n)


def test_occlusion_without_the_knob_is_what_it_was(rsdsfm, clip):
    """the knob set back to 0 and occlusion = 1 against the same call on a fresh context that never touched the knob: the library against
    itself at a setting it already had, on purpose -- a no-change check only"""
    import torch

    n = len(clip["data"][0]) - 1
    _equal_runs(_clip_run(rsdsfm, torch, clip, "one", knob=0), _clip_run(rsdsfm, torch, clip, "one", knob=None), n)


def test_the_fold_clip_recovers_pixels_and_leaves_no_more_empty(rsdsfm, clip):
    """on the fold clip at least one pixel is recovered (counted by the public frame calls: on these tiny solved clips the recoveries fall on
    the blend's layers, where every pixel of a neighbour is offered; the fill and the crop offer only the own frame's empty band), and on both
    clips `none` does not rise against occlusion = 1 alone: a candidate's decisions do not depend on the mask, so with the search every
    frame's mask holds at least what it held without"""
    import torch

    parts, on, off = _clip_run(rsdsfm, torch, clip, "parts"), _clip_run(rsdsfm, torch, clip, "one", knob=1), _clip_run(rsdsfm, torch, clip, "one", knob=None)
    print(clip["name"], "recovered (filled, cropped, blend layers)", parts["recovered"], "rejected", parts["rejected"], "none with the search", on["counts"][:, 0].tolist(), on["crop_counts"][:, 0].tolist(),
          "without", off["counts"][:, 0].tolist(), off["crop_counts"][:, 0].tolist())
    for key in ("counts", "crop_counts"):
        assert (on[key][:, 0] <= off[key][:, 0]).all(), key
    if clip["name"].startswith("fold"):
        assert sum(parts["recovered"]) >= 1 and parts["rejected"][0] >= 1 and parts["rejected"][1] >= 1


def test_evaluate_real_sequence_with_the_search(rsdsfm, clip, tmp_path):
    """evaluate_real_sequence(..., occlusion=True, occlusion_search=True): the keys of the call without the keyword plus the recovered sums,
    which are the frame calls' own counters and go to occlusion_search.csv; the keyword needs occlusion"""
    frames, rows, cols, K, gamma, seeds, window_in = clip["data"]
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0, fill=2, crop=True, crop_margin=0, crop_max_empty=npix_allowed(rows, cols),
              occlusion=True, occlusion_tol=TOL)
    n = len(frames) - 1
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, occlusion_search=True, out_dir=str(tmp_path), **kw)
        plain = ev(s, frames, **kw)
        with pytest.raises(ValueError, match="occlusion"):
            ev(s, frames, occlusion_search=True, **dict(kw, occlusion=False))
        ps, again = out["path_smoothed"], []
        for p in range(n):  # every filled frame as Solver.stabilize_search gives it candidate after candidate
            img, mask = out["stabilized"][p], out["stab_masks"][p]
            source, counts, recovered = mask.copy(), [0, int(mask.sum()), 0, 0, 0, 0], 0
            for q, sid, nM, nm in zip(*rsdsfm.neighbour_poses(out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], p, 2)):
                o = out["pairs"][int(q)]
                img, mask, source, taken, _, rec = s.stabilize_search(frames[int(q)], o["depth_map"], o["R"], o["t"], K, nM, nm, int(sid), image=img, mask=mask,
                                                                      source=source, tol_q16=int(round(TOL * 65536)))
                counts[int(sid)], recovered = taken + rec, recovered + rec
            counts[0] = rows * cols - sum(counts[1:])
            again.append((img, source, counts, recovered))
    assert set(out) == set(plain) | {"fill_recovered", "crop_recovered"}
    lines = open(os.path.join(str(tmp_path), "occlusion_search.csv")).read().split()
    assert lines[0] == "pair,fill_recovered,crop_recovered" and lines[1:] == ["%d,%d,%d" % (p, out["fill_recovered"][p], out["crop_recovered"][p]) for p in range(n)]
    assert out["fill_recovered"].shape == out["crop_recovered"].shape == (n,) and (out["fill_recovered"] >= 0).all()
    for p in range(n):
        assert np.array_equal(out["stabilized"][p], plain["stabilized"][p])
        for key in ("fill_counts", "crop_counts"):
            assert out[key].shape == plain[key].shape and out[key][p].sum() == rows * cols
        assert out["fill_counts"][p, 0] <= plain["fill_counts"][p, 0]
        assert np.array_equal(out["stab_filled"][p], again[p][0]) and np.array_equal(out["stab_sources"][p], again[p][1])
        assert out["fill_counts"][p].tolist() == again[p][2] and int(out["fill_recovered"][p]) == again[p][3]


def npix_allowed(rows, cols):
    """the crop search of evaluate_real_sequence on these tiny frames: up to a quarter of the frame may stay empty"""
    return rows * cols // 4
