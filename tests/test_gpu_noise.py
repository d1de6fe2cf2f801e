"""GPU: the noise level (include/rsdsfm_noise.h) bit for bit against its definition (tests/noise_spec_numpy.py) in both library builds -- the
primitive's histogram and record at the shapes where its 16 x 64 tile, its byte paths and its halo can go wrong, the accumulate and the top-up
with the strength from a record against the existing calls made with the definition's h, the frame call against the public calls made one after
another, the clip call against the frame calls, evaluate_real_sequence, and the refusals.  Every plane sits at the minimum alignment the header
admits (4 bytes and not 8; the records and counters 8 and not 16) between guard bytes (tests/guarded_planes.py); the outputs are never preset
and the inputs are verified unchanged."""
import os

import numpy as np
import pytest

import denoise_cases as dcases
import denoise_spatial_cases as scases
import noise_cases as cases
import noise_spec_numpy as spec
from guarded_planes import Plane, fresh

pytestmark = pytest.mark.gpu


def _dev(torch):
    return torch.device("cuda", 0)


def _record(n, m):
    return np.array([n, m, (256000 * m + 2023) // 4047, 0], dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------
# the primitive
# ---------------------------------------------------------------------------------------------------
def _level(torch, s, image, mask, quantile_q8=0):
    dev = _dev(torch)
    rows, cols = mask.shape
    p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
    o_h, o_r = fresh((spec.BINS,), np.uint32, 4, device=dev), fresh((4,), np.uint64, 8, device=dev)
    s.noise_level_dev(p_i.ptr, p_m.ptr, 1 if image.ndim == 2 else 3, rows, cols, o_h.ptr, o_r.ptr, quantile_q8)
    s.synchronize()
    assert p_i.unchanged() and p_m.unchanged()
    return dict(hist=o_h.get(), record=o_r.get())


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_primitive_equals_the_definition(rsdsfm, arith):
    """every shape of noise_cases.SHAPES x one and three channels x noisy, holes, clipped, flat (the contention path) and checker (the clamp
    bin), the quantile at the default, 1, 128 and 256"""
    import torch

    with rsdsfm.Solver(0, arith=arith) as s:
        every = cases.primitive_cases()
        assert {c["image"].shape[:2] for c in every} == set(cases.SHAPES)
        for case in every:
            want = cases.run_spec(case)
            got = _level(torch, s, case["image"], case["mask"], case["quantile_q8"])
            assert np.array_equal(got["hist"], want["hist"]), case["name"]
            assert got["record"].tolist() == want["record"].tolist(), (case["name"], got["record"], want["record"])
        assert rsdsfm.noise_level_launches() == 2
        case = every[-7]
        r = s.noise_level(case["image"], case["mask"], 200)  # the host convenience
        want = spec.noise_level(case["image"], case["mask"], 200)
        assert np.array_equal(r["hist"], want["hist"]) and r["record"].tolist() == want["record"].tolist() and r["sigma"] == spec.sigma(want["record"])


def test_primitive_argument_errors(rsdsfm):
    """every refusal is RSDSFM_ERR_INVALID with a "noise level: " message and enqueues nothing: the outputs keep their guard bytes; after a
    refused call the same call without the fault goes through"""
    import torch

    dev = _dev(torch)
    rows, cols = 16, 64
    image, mask = cases.frame(rows, cols, 3, "holes", seed=2)
    p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
    o_h, o_r = fresh((spec.BINS,), np.uint32, 4, device=dev), fresh((4,), np.uint64, 8, device=dev)
    with rsdsfm.Solver(0) as s:
        def call(i=p_i.ptr, m=p_m.ptr, ch=3, r=rows, c=cols, h=o_h.ptr, rec=o_r.ptr, q=0):
            return s.noise_level_dev(i, m, ch, r, c, h, rec, q)

        bads = (dict(i=0), dict(m=0), dict(h=0), dict(rec=0), dict(i=p_i.ptr + 1), dict(m=p_m.ptr + 2), dict(h=o_h.ptr + 2), dict(rec=o_r.ptr + 4), dict(h=p_i.ptr),
                dict(h=p_m.ptr), dict(h=o_r.ptr), dict(rec=p_i.ptr), dict(ch=2), dict(ch=4), dict(r=1), dict(c=1), dict(r=16385), dict(c=16385), dict(q=-1), dict(q=257))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError, match="noise level: "):
                call(**bad)
        s.synchronize()
        assert o_h.unchanged() and o_r.unchanged()  # nothing was enqueued
        with pytest.raises(rsdsfm.RsdsfmError):
            call(i=0)
        call()
        s.synchronize()
        want = spec.noise_level(image, mask)
        assert np.array_equal(o_h.get(), want["hist"]) and o_r.get().tolist() == want["record"].tolist() and p_i.unchanged() and p_m.unchanged()


# ---------------------------------------------------------------------------------------------------
# the accumulate and the top-up with the strength from a record
# ---------------------------------------------------------------------------------------------------
# (record, fallback, scale, min_samples): h = 12; too few samples: the fallback; m = 0: h = 1; m = 1023: h = 255; a scale and a min_samples of the caller's
RECORDS = [(_record(5000, 16), 0, 0, 0), (_record(1023, 16), 40, 0, 0), (_record(5000, 0), 30, 0, 0), (_record(5000, 1023), 3, 0, 0), (_record(70, 9), 200, 40, 64)]


def _accumulate_chain(torch, s, ref, rmask, layers, records, record4=None, strength=0, scale=0, min_samples=0):
    """the layers one after another through rsdsfm_denoise_accumulate_dev (record4 None) or its auto variant -> dict(image, mask, weight, counts)"""
    dev = _dev(torch)
    rows, cols = rmask.shape
    ch = 1 if ref.ndim == 2 else 3
    p_r, p_m = Plane(ref, 4, device=dev), Plane(rmask, 4, device=dev)
    p_n = Plane(record4, 8, device=dev) if record4 is not None else None
    p_l = [(Plane(i, 4, device=dev), Plane(m, 4, device=dev)) for i, m in layers]
    p_rec = [Plane(r, 8, device=dev) if r is not None else None for r in records]
    cells = fresh((rows, cols, ch + 1), np.uint16, 8, device=dev)
    o = dict(image=fresh(ref.shape, np.uint8, 4, device=dev), mask=fresh((rows, cols), np.uint8, 4, device=dev), weight=fresh((rows, cols), np.uint8, 4, device=dev),
             counts=fresh((3,), np.int64, 8, device=dev))
    outs = dict(d_image_out=o["image"].ptr, d_mask_out=o["mask"].ptr, d_weight=o["weight"].ptr, d_counts3=o["counts"].ptr)
    steps = p_l or [(None, None)]
    for j, (li, lm) in enumerate(steps):
        first, last = j == 0, j == len(steps) - 1
        args = (p_r.ptr, p_m.ptr, li.ptr if li else None, lm.ptr if lm else None, ch, rows, cols, cells.ptr if p_l else None, first, last)
        rec = p_rec[j].ptr if p_l and p_rec[j] is not None else None
        if p_n is None:
            s.denoise_accumulate_dev(*args, rec, 0, 0, strength, **outs)
        else:
            s.denoise_accumulate_auto_dev(*args, p_n.ptr, rec, 0, 0, strength, scale, min_samples, **outs)
    s.synchronize()
    assert p_r.unchanged() and p_m.unchanged() and (p_n is None or p_n.unchanged()) and all(a.unchanged() and b.unchanged() for a, b in p_l)
    return dict(image=o["image"].get(), mask=o["mask"].get(), weight=o["weight"].get(), counts=o["counts"].get().tolist(), cells=cells.get() if len(steps) > 1 else None)


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_auto_accumulate_equals_the_existing_call_at_the_definitions_strength(rsdsfm, arith):
    """no layer (FIRST and LAST), one layer (FIRST and LAST), two (FIRST, then LAST) and three (a mid step) x gray and BGR x the records above:
    every output byte, the counters and the cells a mid step leaves are the existing call's made with h = noise_strength(...)"""
    import torch

    differs = 0
    with rsdsfm.Solver(0, arith=arith) as s:
        for k, (rows, cols) in enumerate([(5, 5), (17, 65), (16, 131)]):
            for ch in (1, 3):
                ref, rmask = dcases.reference(rows, cols, ch, seed=k)
                recs = dcases.records(ch)
                for L in (0, 1, 2, 3):
                    layers = dcases.layers(ref, rows, cols, ch, L, seed=k)
                    records = [list(recs.values())[(j + k) % 5] if (j + L) % 2 else None for j in range(L)]
                    for record4, fallback, scale, min_samples in RECORDS[(k + L) % 2::2] if rows > 5 else RECORDS:
                        h = spec.noise_strength(int(record4[0]), int(record4[1]), scale, fallback or 12, min_samples)
                        assert rsdsfm.noise_strength(int(record4[0]), int(record4[1]), scale, fallback, min_samples) == h
                        want = _accumulate_chain(torch, s, ref, rmask, layers, records, None, h)
                        got = _accumulate_chain(torch, s, ref, rmask, layers, records, record4, fallback, scale, min_samples)
                        for key in ("image", "mask", "weight"):
                            assert np.array_equal(got[key], want[key]), (rows, cols, ch, L, h, key)
                        assert got["counts"] == want["counts"] and (want["cells"] is None or np.array_equal(got["cells"], want["cells"]))
                        if L and h != 12:
                            differs += int(not np.array_equal(want["image"], _accumulate_chain(torch, s, ref, rmask, layers, records, None, 12)["image"]))
    assert differs > 0  # the strength matters on these inputs


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_auto_top_up_equals_the_existing_call_at_the_definitions_strength(rsdsfm, arith):
    import torch

    dev = _dev(torch)
    with rsdsfm.Solver(0, arith=arith) as s:
        k = 0
        for rows, cols in [(2, 9), (17, 65), (33, 130)]:
            for ch in (1, 3):
                for S in scases.SEARCHES:
                    image, mask, weight = scases.frame(rows, cols, ch, seed=S)
                    record4, fallback, scale, min_samples = RECORDS[k % len(RECORDS)]
                    weight = weight if k % 3 else None
                    k += 1
                    h = spec.noise_strength(int(record4[0]), int(record4[1]), scale, fallback or 12, min_samples)
                    p_i, p_m, p_n = Plane(image, 4, device=dev), Plane(mask, 4, device=dev), Plane(record4, 8, device=dev)
                    p_w = Plane(weight, 4, device=dev) if weight is not None else None
                    got, want = [], []
                    for auto, res in ((True, got), (False, want)):
                        o_i, o_s, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev), fresh((3,), np.int64, 8, device=dev)
                        if auto:
                            s.denoise_spatial_auto_dev(p_i.ptr, p_m.ptr, p_w.ptr if p_w else None, ch, rows, cols, p_n.ptr, o_i.ptr, o_s.ptr, o_c.ptr, fallback, scale, min_samples, 70, S)
                        else:
                            s.denoise_spatial_dev(p_i.ptr, p_m.ptr, p_w.ptr if p_w else None, ch, rows, cols, o_i.ptr, o_s.ptr, o_c.ptr, h, 70, S)
                        s.synchronize()
                        res += [o_i.get(), o_s.get(), o_c.get().tolist()]
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (rows, cols, ch, S, h)
                    assert p_i.unchanged() and p_m.unchanged() and p_n.unchanged() and (p_w is None or p_w.unchanged())
        image, mask, weight = scases.frame(17, 65, 3, seed=4)  # the host conveniences
        img, sup, counts = s.denoise_spatial_auto(image, mask, _record(5000, 40), weight, target=100, search=3)
        img2, sup2, counts2 = s.denoise_spatial(image, mask, weight, strength=30, target=100, search=3)
        assert np.array_equal(img, img2) and np.array_equal(sup, sup2) and counts.tolist() == counts2.tolist()
        ref, rmask = dcases.reference(17, 65, 3)
        layers = dcases.layers(ref, 17, 65, 3, 2)
        a = s.denoise_accumulate_auto(ref, rmask, layers, _record(5000, 40))
        b = s.denoise_accumulate(ref, rmask, layers, strength=30)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_auto_primitive_argument_errors(rsdsfm):
    """the refusals the record, the scale and min_samples add; nothing is enqueued"""
    import torch

    dev = _dev(torch)
    rows, cols = 16, 64
    image, mask, weight = scases.frame(rows, cols, 3, seed=2)
    ref, rmask = dcases.reference(rows, cols, 3)
    (limg, lmask), = dcases.layers(ref, rows, cols, 3, 1)
    P = lambda a, al=4: Plane(a, al, device=dev)
    p_i, p_m, p_w, p_n, p_r, p_rm, p_l, p_lm = P(image), P(mask), P(weight), P(_record(5000, 16), 8), P(ref), P(rmask), P(limg), P(lmask)
    o_i, o_k, o_s, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev), fresh(
        (3,), np.int64, 8, device=dev)
    with rsdsfm.Solver(0) as s:
        def top_up(n=p_n.ptr, o=o_i.ptr, sp=o_s.ptr, cnt=o_c.ptr, h=0, scale=0, ms=0, target=0, search=0):
            return s.denoise_spatial_auto_dev(p_i.ptr, p_m.ptr, p_w.ptr, 3, rows, cols, n, o, sp, cnt, h, scale, ms, target, search)

        def accumulate(n=p_n.ptr, o=o_i.ptr, cnt=o_c.ptr, h=0, scale=0, ms=0, first=True, last=True):
            return s.denoise_accumulate_auto_dev(p_r.ptr, p_rm.ptr, p_l.ptr, p_lm.ptr, 3, rows, cols, None, first, last, n, None, 0, 0, h, scale, ms, o, o_k.ptr, o_s.ptr, cnt)

        for bad in (dict(n=0), dict(n=p_n.ptr + 4), dict(n=o_i.ptr), dict(cnt=p_n.ptr), dict(scale=256), dict(scale=-1), dict(ms=-1), dict(h=256), dict(h=-1), dict(target=256),
                    dict(search=4), dict(o=p_i.ptr)):
            with pytest.raises(rsdsfm.RsdsfmError, match="denoise spatial auto: "):
                top_up(**bad)
        for bad in (dict(n=0), dict(n=p_n.ptr + 4), dict(o=p_n.ptr), dict(cnt=p_n.ptr), dict(scale=256), dict(scale=-1), dict(ms=-1), dict(h=256), dict(h=-1), dict(first=False),
                    dict(o=p_r.ptr)):
            with pytest.raises(rsdsfm.RsdsfmError, match="denoise auto"):
                accumulate(**bad)
        s.synchronize()
        assert o_i.unchanged() and o_k.unchanged() and o_s.unchanged() and o_c.unchanged()
        top_up()
        s.synchronize()
        want = s.denoise_spatial(image, mask, weight)
        assert np.array_equal(o_i.get(), want[0]) and np.array_equal(o_s.get(), want[1]) and o_c.get().tolist() == want[2].tolist()


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
SPATIAL = dict(spatial=True, spatial_strength=120, target=60, search=3)
NOISE = dict(scale=40, min_samples=64)  # the cases are small: 1024 samples are more than some of them have


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
    return dict(image=fresh(case["frames"][0].shape, np.uint8, 4, device=dev), mask=plane(), weight=plane(), support=plane(), counts=fresh((6,), np.int64, 8, device=dev),
                noise=fresh((4,), np.uint64, 8, device=dev))


def _collect(o, top_up, with_optional=True):
    assert top_up or o["support"].unchanged()
    assert with_optional or (o["weight"].unchanged() and o["support"].unchanged() and o["counts"].unchanged() and o["noise"].unchanged())
    return dict(image=o["image"].get(), mask=o["mask"].get(), weight=o["weight"].get() if with_optional else None, support=o["support"].get() if top_up and with_optional else None,
                counts=o["counts"].get().tolist() if with_optional else None, noise=o["noise"].get().tolist() if with_optional else None)


def _same_frame(got, want, name=""):
    for k in ("image", "mask", "weight", "support"):
        assert got[k] is None or np.array_equal(got[k], want[k]), (name, k)
    for k in ("counts", "noise"):
        assert got[k] is None or list(got[k]) == list(want[k]), (name, k, got[k], want[k])


def _frame(torch, s, case, d=None, q=None, top_up=False, with_optional=True, noise=NOISE):
    """one rsdsfm_denoise_auto_frame_dev of frame q of a case into guarded, never preset outputs"""
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = d or _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case, q)
    o = _outputs(dev, case)
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    opt = lambda k: o[k].ptr if with_optional else None
    s.set_occlusion_search(case["search"])
    s.denoise_auto_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, o["image"].ptr, o["mask"].ptr, opt("weight"),
                             opt("support") if top_up else None, opt("counts"), opt("noise"), **_frame_kw(case), **noise, **(SPATIAL if top_up else {}))
    s.synchronize()
    s.set_occlusion_search(0)
    for t, a in zip(d["frames"], case["frames"]):
        assert np.array_equal(t.cpu().numpy(), a)
    return _collect(o, top_up, with_optional)


def _public_calls(torch, s, rsdsfm, case, d=None, q=None, top_up=False, noise=NOISE):
    """what the frame call promises to equal: the own render, the noise level on it, then the EXISTING frame call (and the existing top-up) made
    with the strength the host forms from the record -- public calls one after another on planes of the test's own"""
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = d or _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case, q)
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    kw = _frame_kw(case)
    s.set_occlusion_search(case["search"])
    # the rendered reference planes: the existing frame call on the own frame alone gives (R, mR) as its image and mask
    ref, rmask = fresh(case["frames"][0].shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev)
    s.denoise_frame_dev(pick("frames")[:1], ch, pick("maps")[:1], pick("Rs")[:1], pick("ts")[:1], case["K"], rows, cols, M[:1], m[:1], ref.ptr, rmask.ptr, **kw)
    hist, rec = fresh((spec.BINS,), np.uint32, 4, device=dev), fresh((4,), np.uint64, 8, device=dev)
    s.noise_level_dev(ref.ptr, rmask.ptr, ch, rows, cols, hist.ptr, rec.ptr)
    s.synchronize()
    record = rec.get()
    want = spec.noise_level(ref.get(), rmask.get())
    assert record.tolist() == want["record"].tolist() and np.array_equal(hist.get(), want["hist"])
    h = rsdsfm.noise_strength(int(record[0]), int(record[1]), noise["scale"], case["strength"], noise["min_samples"])
    o = _outputs(dev, case)
    mid = fresh(case["frames"][0].shape, np.uint8, 4, device=dev)
    c3 = [fresh((3,), np.int64, 8, device=dev) for _ in range(2)]
    s.denoise_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, mid.ptr if top_up else o["image"].ptr, o["mask"].ptr, o["weight"].ptr,
                        c3[0].ptr, **dict(kw, strength=h))
    counts = [0, 0, 0]
    if top_up:
        hs = rsdsfm.noise_strength(int(record[0]), int(record[1]), noise["scale"], SPATIAL["spatial_strength"], noise["min_samples"])
        s.denoise_spatial_dev(mid.ptr, o["mask"].ptr, o["weight"].ptr, ch, rows, cols, o["image"].ptr, o["support"].ptr, c3[1].ptr, hs, SPATIAL["target"], SPATIAL["search"])
    s.synchronize()
    s.set_occlusion_search(0)
    if top_up:
        counts = c3[1].get().tolist()
    return dict(image=o["image"].get(), mask=o["mask"].get(), weight=o["weight"].get(), support=o["support"].get() if top_up else None,
                counts=c3[0].get().tolist() + counts, noise=record.tolist(), h=h)


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_frame_call_equals_the_public_calls(oracle, rsdsfm, arith):
    """every frame case of tests/denoise_cases.py -- the noisy shift scene, a fold pair plain, through the occlusion test and through the search, a
    zoomed window, gained neighbours with the gain on, off and under too small an overlap, five sources from the clip's middle and one-sided from
    its ends, one source, the 2 x 2 dense case (no sample: the fallback) -- with and without the top-up, with and without the optional outputs"""
    import torch

    every = {c["name"]: c for c in dcases.all_cases(oracle.pose_table)}
    assert len(every) == 14 and {"fold-visible", "fold-search", "fold-zoom", "gained", "gain-off", "gain-small-overlap", "five-radius-7", "one-source", "2x2"} <= set(every)
    strengths = set()
    with rsdsfm.Solver(0, arith=arith) as s:
        for name, case in every.items():
            rows, cols = case["depths"][0].shape
            nsrc = len(dcases.sources_and_poses(case)[0])
            assert (nsrc == 1) == (name == "one-source")
            for top_up in (False, True):
                want = _public_calls(torch, s, rsdsfm, case, top_up=top_up)
                strengths.add(want["h"])
                _same_frame(_frame(torch, s, case, top_up=top_up), want, (name, top_up))
                _same_frame(_frame(torch, s, case, top_up=top_up, with_optional=False), want, (name, top_up, "bare"))
                assert rsdsfm.denoise_auto_frame_launches(rows, cols, nsrc, top_up) == rsdsfm.denoise_launches(rows, cols, nsrc) + 2 + int(top_up)
        case = every["fold-plain"]  # the defaults: 1024 samples or the fallback
        _same_frame(_frame(torch, s, case, noise=dict()), _public_calls(torch, s, rsdsfm, case, noise=dict(scale=0, min_samples=0)), "defaults")
    assert len(strengths) > 2  # the cases ask for different strengths


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
        def call(images=pick("frames"), maps=pick("maps"), M=M, m=m, i=o["image"].ptr, k=o["mask"].ptr, w=o["weight"].ptr, sp=o["support"].ptr, cnt=o["counts"].ptr,
                 nz=o["noise"].ptr, ch=3, spatial=True, **kw):
            return s.denoise_auto_frame_dev(images, ch, maps, pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, i, k, w, sp, cnt, nz, spatial=spatial, **kw)

        bad_M = M.copy()
        bad_M[1, 0, 0] = np.nan
        params, sparams, nparams = rsdsfm.DenoiseParams(), rsdsfm.DenoiseSpatialParams(), rsdsfm.NoiseParams()
        params.struct_bytes, sparams.struct_bytes, nparams.struct_bytes = 40, 28, 32
        bads = (dict(images=[0] + pick("frames")[1:]), dict(maps=pick("maps")[:1] + [0]), dict(images=[]), dict(M=bad_M), dict(i=0), dict(k=0), dict(i=o["mask"].ptr),
                dict(w=o["image"].ptr), dict(sp=o["image"].ptr), dict(sp=o["weight"].ptr), dict(i=o["image"].ptr + 1), dict(sp=o["support"].ptr + 2), dict(cnt=o["counts"].ptr + 4),
                dict(cnt=o["image"].ptr), dict(i=pick("frames")[1]), dict(ch=2), dict(strength=256), dict(occlusion=2), dict(window=(0, 0, rows + 1, cols)), dict(iterations=17),
                dict(params=params), dict(spatial_params=sparams), dict(noise_params=nparams), dict(spatial_strength=256), dict(target=256), dict(search=4), dict(spatial=False),
                dict(nz=o["noise"].ptr + 4), dict(nz=o["counts"].ptr), dict(nz=o["image"].ptr), dict(nz=pick("frames")[0]), dict(nz=pick("maps")[1]), dict(nz=d["Rs"][src[0]].data_ptr()), dict(nz=d["ts"][src[1]].data_ptr()), dict(quantile_q8=257), dict(quantile_q8=-1),
                dict(scale=256), dict(scale=-1), dict(min_samples=-1))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        assert all(p.unchanged() for p in o.values())
        call(strength=case["strength"], **NOISE, **SPATIAL)
        s.synchronize()
        _same_frame(_collect(o, True), _public_calls(torch, s, rsdsfm, case, top_up=True))


# ---------------------------------------------------------------------------------------------------
# the clip call
# ---------------------------------------------------------------------------------------------------
def _video(torch, s, case, top_up, want_counts=True, want_noise=True, with_optional=True):
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    ns = len(case["depths"])
    d = _clip(torch, dev, case)
    outs = [_outputs(dev, case) for _ in range(ns)]
    ptrs = lambda a: [x.data_ptr() for x in a]
    col = lambda k: [o[k].ptr for o in outs]
    r = s.denoise_auto_video_dev(ptrs(d["frames"]), rows, cols, ch, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"], case["c_path"],
                                 case["scales"], col("image"), col("mask"), col("weight") if with_optional else None, col("support") if with_optional and top_up else None,
                                 want_counts=want_counts, want_noise=want_noise, radius=case["radius"], **_frame_kw(case), **NOISE, **(SPATIAL if top_up else {}))
    s.synchronize()
    got = []
    for q, o in enumerate(outs):
        assert o["counts"].unchanged() and o["noise"].unchanged() and (top_up and with_optional or o["support"].unchanged()) and (with_optional or o["weight"].unchanged())
        got.append(dict(image=o["image"].get(), mask=o["mask"].get(), weight=o["weight"].get() if with_optional else None,
                        support=o["support"].get() if top_up and with_optional else None, counts=r["counts"][q].tolist() if want_counts else None,
                        noise=r["noise"][q].tolist() if want_noise else None))
    assert set(r) == ({"counts"} if want_counts else set()) | ({"noise"} if want_noise else set())
    return got, d, outs


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_clip_call_equals_the_frame_calls(oracle, rsdsfm, arith):
    """five frames at radius 2 (one-sided neighbours at the ends), a fold pair, a zoomed window, the occlusion test and the gain switched off, with and
    without the top-up: every frame of the clip call is the frame call's, counters and records included; with neither host array the call only
    enqueues; a refused call enqueues nothing"""
    import torch

    every = {c["name"]: c for c in dcases.all_cases(oracle.pose_table)}
    with rsdsfm.Solver(0, arith=arith) as s:
        # beside the two plain clips: a zoomed window, the neighbours through the occlusion test, the gain switched off
        for case, top_up in ((every["shift-bgr-0"], True), (every["fold-plain"], False), (every["fold-zoom"], True), (every["fold-visible"], False), (every["gain-off"], True)):
            got, d, _ = _video(torch, s, case, top_up)
            for q in range(len(case["depths"])):
                _same_frame(got[q], _frame(torch, s, case, d, q, top_up), (case["name"], q))
        case = every["shift-bgr-0"]
        full, _, _ = _video(torch, s, case, True)
        for kw in (dict(want_counts=False), dict(want_noise=False), dict(want_counts=False, want_noise=False, with_optional=False)):
            got, _, _ = _video(torch, s, case, True, **kw)
            for q in range(len(case["depths"])):
                _same_frame(got[q], full[q], (q, kw))
        dev = _dev(torch)
        rows, cols = case["depths"][0].shape
        ns = len(case["depths"])
        d = _clip(torch, dev, case)
        outs = [_outputs(dev, case) for _ in range(ns)]
        ptrs = lambda a: [x.data_ptr() for x in a]
        bad_scales = case["scales"].copy()
        bad_scales[ns - 1] = 0.0

        def call(scales=case["scales"], i=None, sp=None, **kw):
            return s.denoise_auto_video_dev(ptrs(d["frames"]), rows, cols, 3, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"],
                                            case["c_path"], scales, i or [o["image"].ptr for o in outs], [o["mask"].ptr for o in outs], None, sp, **kw)

        for bad in (dict(scales=bad_scales), dict(radius=8), dict(strength=300), dict(spatial=True, search=4), dict(scale=256), dict(quantile_q8=300), dict(min_samples=-1),
                    dict(i=[outs[0]["image"].ptr] * (ns - 1) + [0]), dict(sp=[o["support"].ptr for o in outs]),
                    dict(i=[outs[0]["image"].ptr] * (ns - 1) + [d["frames"][1].data_ptr()])):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        assert all(p.unchanged() for o in outs for p in o.values())


# ---------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------
def test_evaluate_real_sequence_with_the_measured_strength(rsdsfm, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, denoise=(K, "auto"[, spatial])) adds exactly denoise_noise to the keys of the same call with an
    integer strength and three columns to denoise.csv; every frame is the existing call's frame at the strength its own record asks for; with an
    integer strength nothing differs from what it was"""
    from test_gpu_stabilize_search import TRIALS, plain_clip

    frames, rows, cols, K, gamma, seeds, _ = plain_clip(rsdsfm)
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
    n = len(frames) - 1
    with rsdsfm.Solver(0) as s:
        auto = ev(s, frames, denoise=(1, "auto"), out_dir=str(tmp_path / "auto"), **kw)
        topped = ev(s, frames, denoise=(1, "auto", True), **kw)
        plain = ev(s, frames, denoise=(1, 30), out_dir=str(tmp_path / "plain"), **kw)
        assert set(auto) == set(plain) | {"denoise_noise"} and set(topped) == set(auto) | {"denoise_support", "denoise_spatial_counts"}
        noise = auto["denoise_noise"]
        assert noise.shape == (n, 4) and np.array_equal(noise, topped["denoise_noise"]) and (noise[:, 0] > 0).all()
        for p in range(n):
            assert noise[p, 3] == rsdsfm.noise_strength(int(noise[p, 0]), int(noise[p, 1])) and noise[p, 2] == (256000 * noise[p, 1] + 2023) // 4047
        for k in plain:
            if k not in ("pairs", "path_smoothed", "links", "stab_denoised", "denoise_masks", "denoise_weights", "denoise_counts"):
                assert np.asarray(auto[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
        hs = sorted(set(int(h) for h in noise[:, 3]))
        assert 1 <= len(hs) <= n
        for h in hs:  # every frame is the existing call's frame at the strength its own record asks for
            same = ev(s, frames, denoise=(1, h), **kw)
            mine = [p for p in range(n) if int(noise[p, 3]) == h]
            assert mine
            for p in mine:
                for k in ("stab_denoised", "denoise_masks", "denoise_weights", "denoise_counts"):
                    assert np.asarray(auto[k][p]).tobytes() == np.asarray(same[k][p]).tobytes(), (k, p, h)
        with pytest.raises(ValueError):
            ev(s, frames, denoise=(1, "strong"), **kw)
    lines = open(str(tmp_path / "auto" / "denoise.csv")).read().split()
    assert lines[0] == "pair,unset,own_only,averaged,mean_weight,noise_m,sigma,strength" and len(lines) == 1 + n
    assert lines[1].split(",")[5:] == [str(int(noise[0, 1])), "%.4f" % (int(noise[0, 2]) / 256.0), str(int(noise[0, 3]))]
    assert open(str(tmp_path / "plain" / "denoise.csv")).read().split()[0] == "pair,unset,own_only,averaged,mean_weight"
    assert set(os.listdir(str(tmp_path / "auto"))) == set(os.listdir(str(tmp_path / "plain")))
