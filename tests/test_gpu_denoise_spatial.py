"""GPU: the spatial top-up (include/rsdsfm_denoise_spatial.h) bit for bit against its definition (tests/denoise_spatial_spec_numpy.py) in both
library builds -- the primitive at the shapes where its 16 x 64 tile, its byte paths and its halo of search + 1 can go wrong, the extremes, the
impulse's footprint across a tile corner, the early exit, the frame call against the two public calls made one after another and against the
chain of the two definitions, the clip call against the frame calls, evaluate_real_sequence, and the refusals.  Every plane sits at the minimum
alignment the header admits (4 bytes and not 8; the counters 8 and not 16) between guard bytes (tests/guarded_planes.py); the outputs are never
preset and the inputs are verified unchanged."""
import os

import numpy as np
import pytest

import denoise_cases as dcases
import denoise_spatial_cases as cases
import denoise_spatial_spec_numpy as spec
from guarded_planes import Plane, fresh

pytestmark = pytest.mark.gpu


def _dev(torch):
    return torch.device("cuda", 0)


def _spatial(torch, s, image, mask, weight, strength=0, target=0, search=0, with_support=True, with_counts=True):
    """one rsdsfm_denoise_spatial_dev on guarded planes -> dict(image, support or None, counts or None)"""
    dev = _dev(torch)
    rows, cols = mask.shape
    ch = 1 if image.ndim == 2 else 3
    p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
    p_w = Plane(weight, 4, device=dev) if weight is not None else None
    o_i, o_s, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev), fresh((3,), np.int64, 8, device=dev)
    s.denoise_spatial_dev(p_i.ptr, p_m.ptr, p_w.ptr if p_w else None, ch, rows, cols, o_i.ptr, o_s.ptr if with_support else None, o_c.ptr if with_counts else None, strength,
                          target, search)
    s.synchronize()
    assert p_i.unchanged() and p_m.unchanged() and (p_w is None or p_w.unchanged())
    assert with_support or o_s.unchanged()
    assert with_counts or o_c.unchanged()
    return dict(image=o_i.get(), support=o_s.get() if with_support else None, counts=o_c.get().tolist() if with_counts else None)


def _same(got, want, name=""):
    assert np.array_equal(got["image"], want["image"]), (name, "image")
    assert got["support"] is None or np.array_equal(got["support"], want["support"]), (name, "support")
    assert got["counts"] is None or list(got["counts"]) == list(want["counts"]), (name, got["counts"], want["counts"])


# ---------------------------------------------------------------------------------------------------
# the primitive
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_primitive_equals_the_definition(rsdsfm, arith):
    """every shape of denoise_spatial_cases.SHAPES x one and three channels x search 1, 2, 3: random masks with arbitrary non-zero bytes, random
    weight planes and none, strength and target at 1, at 255 and at the defaults; every optional output present and absent"""
    import torch

    seen = np.zeros(3, dtype=np.int64)
    with rsdsfm.Solver(0, arith=arith) as s:
        every = cases.primitive_cases()
        assert {c["image"].shape[:2] for c in every} == set(cases.SHAPES) and {c["weight"] is None for c in every} == {True, False}
        for k, case in enumerate(every):
            want = cases.run_spec(case)
            args = (case["image"], case["mask"], case["weight"], case["strength"], case["target"], case["search"])
            _same(_spatial(torch, s, *args), want, case["name"])
            if k % 4 == 0:
                for with_support, with_counts in ((False, True), (True, False), (False, False)):
                    _same(_spatial(torch, s, *args, with_support=with_support, with_counts=with_counts), want, case["name"])
            seen += np.array(want["counts"])
        assert rsdsfm.denoise_spatial_launches() == 1
    assert (seen > 0).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_the_extremes(rsdsfm, channels):
    """an image of 255 with n = 1, h = 1, target 255, S = 3: the largest numerator; unchanged, support 255 wherever all 48 candidates are inside"""
    import torch

    rows, cols = 17, 65
    sat = np.full((rows, cols) if channels == 1 else (rows, cols, 3), 255, dtype=np.uint8)
    ones = np.ones((rows, cols), dtype=np.uint8)
    with rsdsfm.Solver(0) as s:
        got = _spatial(torch, s, sat, ones, ones, 1, 255, 3)
        _same(got, spec.denoise_spatial(sat, ones, ones, 1, 255, 3))
        assert (got["image"] == 255).all() and (got["support"][3:-3, 3:-3] == 255).all() and got["counts"] == [0, 0, rows * cols]


@pytest.mark.parametrize("channels", [1, 3])
def test_the_impulse_shows_its_footprint_across_a_tile_corner(rsdsfm, channels):
    """one pixel changed in a flat noisy image, at columns 63 / 64 and rows 15 / 16: the outputs change only inside the (2 S + 1 + 2)^2 window
    about it, and are the definition's -- a halo bug shows"""
    import torch

    rows, cols = 33, 130
    rng = np.random.default_rng(8)
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    flat = (120 + rng.integers(-2, 3, size=shape)).astype(np.uint8)
    ones = np.ones((rows, cols), dtype=np.uint8)
    with rsdsfm.Solver(0) as s:
        for S in cases.SEARCHES:
            base = _spatial(torch, s, flat, ones, None, 12, 80, S)
            _same(base, spec.denoise_spatial(flat, ones, None, 12, 80, S), S)
            for y, x in ((15, 63), (16, 64), (15, 64), (16, 63)):
                image = flat.copy()
                image[y, x] = image[y, x] ^ 0x40
                got = _spatial(torch, s, image, ones, None, 12, 80, S)
                _same(got, spec.denoise_spatial(image, ones, None, 12, 80, S), (S, y, x))
                changed = (got["image"] != base["image"]) if channels == 1 else (got["image"] != base["image"]).any(axis=-1)
                changed |= got["support"] != base["support"]
                ys, xs = np.nonzero(changed)
                assert changed[y, x] and np.abs(ys - y).max() <= S + 1 and np.abs(xs - x).max() <= S + 1, (S, y, x)


@pytest.mark.parametrize("channels", [1, 3])
def test_the_early_exit(rsdsfm, channels):
    """weights all at or above the target: the input's bytes under the mask and [unset, kept, 0]; exactly one tile with one deficient pixel: the
    definition's"""
    import torch

    rows, cols = 33, 130
    image, mask, weight = cases.frame(rows, cols, channels, seed=21)
    weight = np.maximum(weight, 80)
    v = mask != 0
    with rsdsfm.Solver(0) as s:
        for S in cases.SEARCHES:
            got = _spatial(torch, s, image, mask, weight, 12, 80, S)
            assert np.array_equal(got["image"], np.where(v if channels == 1 else v[..., None], image, 0)) and np.array_equal(got["support"], np.where(v, weight, 0))
            assert got["counts"] == [int((~v).sum()), int(v.sum()), 0]
            _same(got, spec.denoise_spatial(image, mask, weight, 12, 80, S), S)
            one, m1 = weight.copy(), mask.copy()
            one[20, 70], m1[20, 70] = 10, 1
            want = spec.denoise_spatial(image, m1, one, 40, 80, S)
            assert want["counts"][2] == 1
            _same(_spatial(torch, s, image, m1, one, 40, 80, S), want, (S, "one deficient pixel"))
        got = _spatial(torch, s, image, mask, None, 12, 16, 2)  # no weight plane: n = 16 reaches a target of 16
        assert got["counts"] == [int((~v).sum()), int(v.sum()), 0] and np.array_equal(got["support"], np.where(v, 16, 0))


def test_the_host_convenience(rsdsfm):
    image, mask, weight = cases.frame(17, 65, 3, seed=4)
    with rsdsfm.Solver(0) as s:
        img, sup, counts = s.denoise_spatial(image, mask, weight, strength=30, target=100, search=3)
        _same(dict(image=img, support=sup, counts=counts.tolist()), spec.denoise_spatial(image, mask, weight, 30, 100, 3))
        img, sup, counts = s.denoise_spatial(image[..., 1], mask)
        _same(dict(image=img, support=sup, counts=counts.tolist()), spec.denoise_spatial(image[..., 1], mask))


def test_primitive_argument_errors(rsdsfm):
    """every refusal is RSDSFM_ERR_INVALID with a "denoise spatial: " message and enqueues nothing: the outputs keep their guard bytes; after a
    refused call the same call without the fault goes through"""
    import torch

    dev = _dev(torch)
    rows, cols = 16, 64
    image, mask, weight = cases.frame(rows, cols, 3, seed=2)
    p_i, p_m, p_w = Plane(image, 4, device=dev), Plane(mask, 4, device=dev), Plane(weight, 4, device=dev)
    o_i, o_s, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev), fresh((3,), np.int64, 8, device=dev)
    with rsdsfm.Solver(0) as s:
        def call(i=p_i.ptr, m=p_m.ptr, w=p_w.ptr, ch=3, r=rows, c=cols, o=o_i.ptr, sp=o_s.ptr, cnt=o_c.ptr, h=0, target=0, search=0):
            return s.denoise_spatial_dev(i, m, w, ch, r, c, o, sp, cnt, h, target, search)

        bads = (dict(i=0), dict(m=0), dict(o=0), dict(i=p_i.ptr + 1), dict(m=p_m.ptr + 2), dict(w=p_w.ptr + 3), dict(o=o_i.ptr + 1), dict(sp=o_s.ptr + 2),
                dict(cnt=o_c.ptr + 4), dict(o=p_i.ptr), dict(o=p_m.ptr), dict(o=p_w.ptr), dict(sp=p_i.ptr), dict(sp=p_m.ptr), dict(sp=p_w.ptr), dict(sp=o_i.ptr),
                dict(ch=2), dict(ch=4), dict(r=1), dict(c=1), dict(r=16385), dict(c=16385), dict(h=-1), dict(h=256), dict(target=-1), dict(target=256), dict(search=-1),
                dict(search=4))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError, match="denoise spatial: "):
                call(**bad)
        s.synchronize()
        assert o_i.unchanged() and o_s.unchanged() and o_c.unchanged()  # nothing was enqueued
        for bad in bads[:3]:
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
            call()  # the same call without the fault goes through
        s.synchronize()
        _same(dict(image=o_i.get(), support=o_s.get(), counts=o_c.get().tolist()), spec.denoise_spatial(image, mask, weight))
        assert p_i.unchanged() and p_m.unchanged() and p_w.unchanged()


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
FRAME_CASES = ("2x2", "shift-bgr-0", "shift-gray-1", "fold-plain")  # the smallest of tests/denoise_cases.py
SPATIAL = dict(spatial_strength=120, target=60, search=3)  # the shift scenes are random textures: at the default strength nothing is similar


def _clip(torch, dev, case):
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(frames=[tt(x) for x in case["frames"]], maps=[tt(z.T) for z in case["depths"]], Rs=[tt(np.asarray(R).reshape(-1, 9)) for R in case["Rs"]],
                ts=[tt(t) for t in case["ts"]])


def _frame_kw(case):
    return dict(strength=case["strength"], gain=case["gain_mode"] == 0, min_overlap=case["min_overlap"], window=case["window"], occlusion=case["occlusion"],
                occlusion_tol_q16=case["tol_q16"], mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])


def _outputs(dev, case):
    rows, cols = case["depths"][0].shape
    plane = lambda: fresh((rows, cols), np.uint8, 4, device=dev)
    return dict(image=fresh(case["frames"][0].shape, np.uint8, 4, device=dev), mask=plane(), weight=plane(), support=plane(), counts=fresh((6,), np.int64, 8, device=dev))


def _collect(o, with_weight=True, with_support=True, with_counts=True):
    assert (with_weight or o["weight"].unchanged()) and (with_support or o["support"].unchanged()) and (with_counts or o["counts"].unchanged())
    return dict(image=o["image"].get(), mask=o["mask"].get(), weight=o["weight"].get() if with_weight else None, support=o["support"].get() if with_support else None,
                counts=o["counts"].get().tolist() if with_counts else None)


def _same_frame(got, want, name=""):
    for k in ("image", "mask", "weight", "support"):
        assert got[k] is None or np.array_equal(got[k], want[k]), (name, k)
    assert got["counts"] is None or list(got["counts"]) == list(want["counts"]), (name, got["counts"], want["counts"])


def _frame(torch, s, case, d=None, q=None, with_weight=True, with_support=True, with_counts=True, spatial=SPATIAL):
    """one rsdsfm_denoise_spatial_frame_dev of frame q of a case into guarded, never preset outputs"""
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = d or _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case, q)
    o = _outputs(dev, case)
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    s.denoise_spatial_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, o["image"].ptr, o["mask"].ptr,
                                o["weight"].ptr if with_weight else None, o["support"].ptr if with_support else None, o["counts"].ptr if with_counts else None,
                                **_frame_kw(case), **spatial)
    s.synchronize()
    for t, a in zip(d["frames"], case["frames"]):
        assert np.array_equal(t.cpu().numpy(), a)
    return _collect(o, with_weight, with_support, with_counts)


def _two_calls(torch, s, case, d=None, q=None, spatial=SPATIAL):
    """the two public calls one after another on planes of the test's own"""
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = d or _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case, q)
    o = _outputs(dev, case)
    mid = fresh(case["frames"][0].shape, np.uint8, 4, device=dev)
    c3 = [fresh((3,), np.int64, 8, device=dev) for _ in range(2)]
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    s.denoise_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, mid.ptr, o["mask"].ptr, o["weight"].ptr, c3[0].ptr, **_frame_kw(case))
    s.denoise_spatial_dev(mid.ptr, o["mask"].ptr, o["weight"].ptr, ch, rows, cols, o["image"].ptr, o["support"].ptr, c3[1].ptr, spatial["spatial_strength"], spatial["target"],
                          spatial["search"])
    s.synchronize()
    r = _collect(o, with_counts=False)
    return dict(r, counts=c3[0].get().tolist() + c3[1].get().tolist())


def _spec_chain(case, q=None, spatial=SPATIAL):
    t = dcases.run_spec(case, q)
    r = spec.denoise_spatial(t["image"], t["mask"], t["weight"], spatial["spatial_strength"], spatial["target"], spatial["search"])
    return dict(image=r["image"], mask=t["mask"], weight=t["weight"], support=r["support"], counts=list(t["counts"]) + list(r["counts"]))


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_frame_call_equals_the_two_public_calls_and_the_definitions(oracle, rsdsfm, arith):
    import torch

    every = {c["name"]: c for c in dcases.all_cases(oracle.pose_table)}
    with rsdsfm.Solver(0, arith=arith) as s:
        for name in FRAME_CASES:
            case = every[name]
            want = _spec_chain(case)
            assert want["counts"][5] > 0
            _same_frame(_frame(torch, s, case), want, name)
            _same_frame(_two_calls(torch, s, case), want, name + " two calls")
            for with_weight, with_support, with_counts in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
                _same_frame(_frame(torch, s, case, None, None, with_weight, with_support, with_counts), want, (name, with_weight, with_support, with_counts))
            rows, cols = case["depths"][0].shape
            nsrc = len(dcases.sources_and_poses(case)[0])
            assert rsdsfm.denoise_spatial_frame_launches(rows, cols, nsrc) == rsdsfm.denoise_launches(rows, cols, nsrc) + 1
        case = every["fold-plain"]  # the top-up's defaults
        t = dcases.run_spec(case)
        r = spec.denoise_spatial(t["image"], t["mask"], t["weight"])
        _same_frame(_frame(torch, s, case, spatial=dict()), dict(image=r["image"], mask=t["mask"], weight=t["weight"], support=r["support"], counts=list(t["counts"]) + list(r["counts"])))


def test_frame_argument_errors(oracle, rsdsfm):
    """a refused frame call enqueues nothing: the outputs keep their guard bytes"""
    import torch

    dev = _dev(torch)
    case = [c for c in dcases.all_cases(oracle.pose_table) if c["name"] == "fold-plain"][0]
    rows, cols = case["depths"][0].shape
    d = _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case)
    o = _outputs(dev, case)
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    with rsdsfm.Solver(0) as s:
        def call(images=pick("frames"), maps=pick("maps"), M=M, m=m, i=o["image"].ptr, k=o["mask"].ptr, w=o["weight"].ptr, sp=o["support"].ptr, cnt=o["counts"].ptr, ch=3, **kw):
            return s.denoise_spatial_frame_dev(images, ch, maps, pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, i, k, w, sp, cnt, **kw)

        bad_M = M.copy()
        bad_M[1, 0, 0] = np.nan
        params, sparams = rsdsfm.DenoiseParams(), rsdsfm.DenoiseSpatialParams()
        params.struct_bytes, sparams.struct_bytes = 40, 28
        bads = (dict(images=[0] + pick("frames")[1:]), dict(maps=pick("maps")[:1] + [0]), dict(images=[]), dict(M=bad_M), dict(i=0), dict(k=0), dict(i=o["mask"].ptr),
                dict(w=o["image"].ptr), dict(sp=o["image"].ptr), dict(sp=o["weight"].ptr), dict(sp=o["mask"].ptr), dict(i=o["image"].ptr + 1), dict(sp=o["support"].ptr + 2),
                dict(cnt=o["counts"].ptr + 4), dict(cnt=o["image"].ptr), dict(i=pick("frames")[1]), dict(sp=pick("frames")[0]), dict(ch=2), dict(strength=256), dict(occlusion=2),
                dict(window=(0, 0, rows + 1, cols)), dict(iterations=17), dict(params=params), dict(spatial_params=sparams), dict(spatial_strength=256), dict(spatial_strength=-1),
                dict(target=256), dict(target=-1), dict(search=4), dict(search=-1))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        assert all(p.unchanged() for p in o.values())
        call(strength=case["strength"], **SPATIAL)
        s.synchronize()
        _same_frame(_collect(o), _spec_chain(case))


# ---------------------------------------------------------------------------------------------------
# the clip call
# ---------------------------------------------------------------------------------------------------
def _video(torch, s, case, want_counts=True, with_optional=True, spatial=SPATIAL):
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    ns = len(case["depths"])
    d = _clip(torch, dev, case)
    outs = [_outputs(dev, case) for _ in range(ns)]
    ptrs = lambda a: [x.data_ptr() for x in a]
    col = lambda k: [o[k].ptr for o in outs]
    r = s.denoise_spatial_video_dev(ptrs(d["frames"]), rows, cols, ch, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"],
                                    case["c_path"], case["scales"], col("image"), col("mask"), col("weight") if with_optional else None,
                                    col("support") if with_optional else None, want_counts=want_counts, radius=case["radius"], **_frame_kw(case), **spatial)
    s.synchronize()
    got = []
    for q, o in enumerate(outs):
        one = _collect(o, with_optional, with_optional, False)
        one["counts"] = r["counts"][q].tolist() if want_counts else None
        got.append(one)
    return got, d


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_clip_call_equals_the_frame_calls(oracle, rsdsfm, arith):
    """five frames at radius 2 (one-sided neighbours at the ends) and a fold pair: every frame of the clip call is the frame call's, counts
    included, which is the definitions'; without the counters and the optional planes the call only enqueues; a refused call enqueues nothing"""
    import torch

    every = {c["name"]: c for c in dcases.all_cases(oracle.pose_table)}
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in (every["shift-bgr-0"], every["fold-plain"]):
            got, d = _video(torch, s, case)
            for q in range(len(case["depths"])):
                want = _spec_chain(case, q)
                _same_frame(got[q], want, (case["name"], q))
                _same_frame(_frame(torch, s, case, d, q), want, (case["name"], q, "frame"))
        case = every["shift-bgr-0"]
        got, _ = _video(torch, s, case, want_counts=False, with_optional=False)
        for q in range(len(case["depths"])):
            _same_frame(got[q], _spec_chain(case, q), q)
        dev = _dev(torch)
        rows, cols = case["depths"][0].shape
        ns = len(case["depths"])
        d = _clip(torch, dev, case)
        outs = [_outputs(dev, case) for _ in range(ns)]
        ptrs = lambda a: [x.data_ptr() for x in a]
        bad_scales = case["scales"].copy()
        bad_scales[ns - 1] = 0.0

        def call(scales=case["scales"], i=None, sp=None, **kw):
            return s.denoise_spatial_video_dev(ptrs(d["frames"]), rows, cols, 3, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"],
                                               case["c_path"], scales, i or [o["image"].ptr for o in outs], [o["mask"].ptr for o in outs], None, sp, **kw)

        for bad in (dict(scales=bad_scales), dict(radius=8), dict(radius=-1), dict(strength=300), dict(search=4), dict(target=256), dict(spatial_strength=-1),
                    dict(i=[outs[0]["image"].ptr] * (ns - 1) + [0]), dict(sp=[outs[0]["support"].ptr] * (ns - 1) + [0]),
                    dict(i=[outs[0]["image"].ptr] * (ns - 1) + [d["frames"][1].data_ptr()])):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        assert all(p.unchanged() for o in outs for p in o.values())


# ---------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------
def test_evaluate_real_sequence_with_the_spatial_top_up(rsdsfm, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, denoise=(K, strength, True)) adds exactly denoise_support and denoise_spatial_counts to the
    denoise's keys and three columns to denoise.csv; the temporal planes are what they are without it and the image is the primitive's on
    them; without the third element nothing differs"""
    from test_gpu_stabilize_search import TRIALS, plain_clip

    frames, rows, cols, K, gamma, seeds, _ = plain_clip(rsdsfm)
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
    n = len(frames) - 1
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, denoise=(1, 30, True), out_dir=str(tmp_path / "with"), **kw)
        plain = ev(s, frames, denoise=(1, 30), out_dir=str(tmp_path / "without"), **kw)
        custom = ev(s, frames, denoise=(1, 30, (40, 1)), **kw)
        new = {"denoise_support", "denoise_spatial_counts"}
        assert set(out) == set(plain) | new == set(custom)
        assert len(out["denoise_support"]) == n and out["denoise_spatial_counts"].shape == (n, 3) and out["denoise_counts"].shape == (n, 3)
        for k in plain:
            if k not in ("pairs", "path_smoothed", "links", "stab_denoised"):
                assert np.asarray(out[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
        for p in range(n):
            img, sup, counts = s.denoise_spatial(plain["stab_denoised"][p], plain["denoise_masks"][p], plain["denoise_weights"][p], strength=30)
            assert np.array_equal(out["stab_denoised"][p], img) and np.array_equal(out["denoise_support"][p], sup) and out["denoise_spatial_counts"][p].tolist() == counts.tolist()
            img, sup, counts = s.denoise_spatial(plain["stab_denoised"][p], plain["denoise_masks"][p], plain["denoise_weights"][p], strength=30, target=40, search=1)
            assert np.array_equal(custom["stab_denoised"][p], img) and custom["denoise_spatial_counts"][p].tolist() == counts.tolist()
            assert out["denoise_spatial_counts"][p].sum() == rows * cols
        assert sum(int(c[2]) for c in out["denoise_spatial_counts"]) > 0  # something was smoothed
    with_files, without_files = set(os.listdir(str(tmp_path / "with"))), set(os.listdir(str(tmp_path / "without")))
    assert with_files == without_files
    lines = open(str(tmp_path / "with" / "denoise.csv")).read().split()
    assert lines[0] == "pair,unset,own_only,averaged,mean_weight,kept,smoothed,mean_support" and len(lines) == 1 + n
    assert lines[1].split(",")[:4] == ["0"] + [str(int(x)) for x in out["denoise_counts"][0]] and lines[1].split(",")[5:7] == [str(int(x)) for x in out["denoise_spatial_counts"][0][1:]]
    assert open(str(tmp_path / "without" / "denoise.csv")).read().split()[0] == "pair,unset,own_only,averaged,mean_weight"
