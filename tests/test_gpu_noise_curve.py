"""GPU: the noise curve (include/rsdsfm_noise_curve.h) bit for bit against its definition (tests/noise_curve_spec_numpy.py) in both library
builds -- the primitive's banded histogram and curve at the shapes where its 16 x 64 tile, its byte paths and its halo can go wrong, and against
Solver.noise_level_dev on the same planes; the accumulate and the top-up with the strength per pixel against the definition, against the
EXISTING calls under a hand-made flat curve and under a curve with too few samples; the frame call against the public calls made one after
another; the clip call against the frame calls; evaluate_real_sequence; and the refusals.  Every plane sits at the minimum alignment the header
admits (4 bytes and not 8; the curves and counters 8 and not 16) between guard bytes (tests/guarded_planes.py); the outputs are never preset
and the inputs are verified unchanged."""
import os

import numpy as np
import pytest

import denoise_cases as dcases
import denoise_spatial_cases as scases
import noise_curve_cases as cases
import noise_curve_spec_numpy as spec
import noise_spec_numpy as nspec
from guarded_planes import Plane, fresh

pytestmark = pytest.mark.gpu

HIST = (spec.BANDS, spec.BINS)


@pytest.fixture(scope="module")
def nc():
    import rsdsfm_noise_curve

    return rsdsfm_noise_curve


def _dev(torch):
    return torch.device("cuda", 0)


def _lut(curve, fallback, scale, ms, bms):
    return spec.strengths(curve, scale, fallback or 12, ms, bms)


# ---------------------------------------------------------------------------------------------------
# the primitive
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_primitive_equals_the_definition_and_the_noise_level(rsdsfm, nc, arith):
    """every shape of noise_cases.SHAPES x one and three channels x noise_cases' kinds and ramp, two_level and band_edge: the banded histogram
    and the nine rows are the definition's; the bands sum to Solver.noise_level_dev's histogram and row 8 is its record, on the same planes"""
    import torch

    dev = _dev(torch)
    with rsdsfm.Solver(0, arith=arith) as s:
        every = cases.primitive_cases()
        assert {c["image"].shape[:2] for c in every} == set(cases.SHAPES) and {c["kind"] for c in every} == set(cases.KINDS)
        for case in every:
            image, mask = case["image"], case["mask"]
            rows, cols = mask.shape
            ch = 1 if image.ndim == 2 else 3
            want = cases.run_spec(case)
            p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
            o_h, o_c = fresh(HIST, np.uint32, 4, device=dev), fresh((9, 4), np.uint64, 8, device=dev)
            o_h1, o_r = fresh((nspec.BINS,), np.uint32, 4, device=dev), fresh((4,), np.uint64, 8, device=dev)
            nc.noise_curve_dev(s, p_i.ptr, p_m.ptr, ch, rows, cols, o_h.ptr, o_c.ptr, case["quantile_q8"])
            s.noise_level_dev(p_i.ptr, p_m.ptr, ch, rows, cols, o_h1.ptr, o_r.ptr, case["quantile_q8"])
            s.synchronize()
            assert p_i.unchanged() and p_m.unchanged()
            hist, curve = o_h.get(), o_c.get()
            assert np.array_equal(hist, want["hist"]), case["name"]
            assert curve.tolist() == want["curve"].tolist(), (case["name"], curve, want["curve"])
            assert np.array_equal(hist.astype(np.uint64).sum(axis=0), o_h1.get().astype(np.uint64)) and curve[8].tolist() == o_r.get().tolist(), case["name"]
        assert nc.noise_curve_launches() == 2
        case = every[-2]
        r = nc.noise_curve(s, case["image"], case["mask"], 200, min_samples=cases.MIN_SAMPLES, band_min_samples=cases.BAND_MIN_SAMPLES)  # the host convenience
        want = spec.noise_curve(case["image"], case["mask"], 200)
        assert np.array_equal(r["hist"], want["hist"]) and r["curve"].tolist() == want["curve"].tolist() and r["sigmas"].tolist() == [int(x) / 256.0 for x in want["curve"][:, 2]]
        assert np.array_equal(r["lut"], spec.strengths(want["curve"], 0, 12, cases.MIN_SAMPLES, cases.BAND_MIN_SAMPLES))


def test_primitive_argument_errors(rsdsfm, nc):
    """every refusal is RSDSFM_ERR_INVALID with a "noise curve: " message and enqueues nothing: the outputs keep their guard bytes; after a
    refused call the same call without the fault goes through"""
    import torch

    dev = _dev(torch)
    rows, cols = 16, 64
    image, mask = cases.frame(rows, cols, 3, "ramp", seed=2)
    p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
    o_h, o_c = fresh(HIST, np.uint32, 4, device=dev), fresh((9, 4), np.uint64, 8, device=dev)
    with rsdsfm.Solver(0) as s:
        def call(i=p_i.ptr, m=p_m.ptr, ch=3, r=rows, c=cols, h=o_h.ptr, cv=o_c.ptr, q=0):
            return nc.noise_curve_dev(s, i, m, ch, r, c, h, cv, q)

        bads = (dict(i=0), dict(m=0), dict(h=0), dict(cv=0), dict(i=p_i.ptr + 1), dict(m=p_m.ptr + 2), dict(h=o_h.ptr + 2), dict(cv=o_c.ptr + 4), dict(h=p_i.ptr),
                dict(h=p_m.ptr), dict(h=o_c.ptr), dict(cv=p_i.ptr), dict(ch=2), dict(ch=4), dict(r=1), dict(c=1), dict(r=16385), dict(c=16385), dict(q=-1), dict(q=257))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError, match="noise curve: "):
                call(**bad)
        s.synchronize()
        assert o_h.unchanged() and o_c.unchanged()  # nothing was enqueued
        call()
        s.synchronize()
        want = spec.noise_curve(image, mask)
        assert np.array_equal(o_h.get(), want["hist"]) and o_c.get().tolist() == want["curve"].tolist() and p_i.unchanged() and p_m.unchanged()


# ---------------------------------------------------------------------------------------------------
# the accumulate and the top-up with the strength per pixel
# ---------------------------------------------------------------------------------------------------
def _accumulate_chain(torch, s, nc, ref, rmask, layers, records, curve=None, strength=0, scale=0, min_samples=0, band_min_samples=0):
    """the layers one after another through rsdsfm_denoise_accumulate_dev (curve None) or its curve variant -> dict(image, mask, weight, counts, cells)"""
    dev = _dev(torch)
    rows, cols = rmask.shape
    ch = 1 if ref.ndim == 2 else 3
    p_r, p_m = Plane(ref, 4, device=dev), Plane(rmask, 4, device=dev)
    p_n = Plane(curve, 8, device=dev) if curve is not None else None
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
            nc.denoise_accumulate_curve_dev(s, *args, p_n.ptr, rec, 0, 0, strength, scale, min_samples, band_min_samples, **outs)
    s.synchronize()
    assert p_r.unchanged() and p_m.unchanged() and (p_n is None or p_n.unchanged()) and all(a.unchanged() and b.unchanged() for a, b in p_l)
    return dict(image=o["image"].get(), mask=o["mask"].get(), weight=o["weight"].get(), counts=o["counts"].get().tolist(), cells=cells.get() if len(steps) > 1 else None)


ACC_SHAPES = [sh for sh in dcases.ACC_SHAPES if sh[0] * sh[1] <= 37 * 67]


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_curve_accumulate_equals_the_definition(rsdsfm, nc, arith):
    """denoise_cases.ACC_SHAPES up to (37, 67) x gray and BGR x no layer, one, two and three layers, on a reference that ramps through every
    level, under the hand-made curves (every band valid, invalid bands, no band valid, too few samples, a caller's scale): every output byte, the
    counters and the cells a mid step leaves are the definition's"""
    import torch

    assert (37, 67) in ACC_SHAPES and (16, 131) in ACC_SHAPES and len(ACC_SHAPES) == 8
    differs = 0
    with rsdsfm.Solver(0, arith=arith) as s:
        for k, (rows, cols) in enumerate(ACC_SHAPES):
            for ch in (1, 3):
                ref, rmask = cases.ramp_reference(rows, cols, ch, seed=k)
                recs = dcases.records(ch)
                for L in (0, 1, 2, 3):
                    layers = dcases.layers(ref, rows, cols, ch, L, seed=k)
                    records = [list(recs.values())[(j + k) % 5] if (j + L) % 2 else None for j in range(L)]
                    curve, fallback, scale, ms, bms = cases.CURVES[(k + L + ch) % len(cases.CURVES)]
                    lut = _lut(curve, fallback, scale, ms, bms)
                    want = spec.denoise(ref, rmask, layers, lut, records)
                    got = _accumulate_chain(torch, s, nc, ref, rmask, layers, records, curve, fallback, scale, ms, bms)
                    for key in ("image", "mask", "weight"):
                        assert np.array_equal(got[key], want[key]), (rows, cols, ch, L, key)
                    assert got["counts"] == want["counts"] and (got["cells"] is None or np.array_equal(got["cells"], want["cells"][-2])), (rows, cols, ch, L)
                    if L and len(set(lut.tolist())) > 1:
                        flat = spec.denoise(ref, rmask, layers, np.full(256, int(np.median(lut)), dtype=np.uint8), records)
                        differs += int(not np.array_equal(flat["image"], want["image"]))
    assert differs > 0  # the strength per pixel matters on these inputs


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_curve_top_up_equals_the_definition(rsdsfm, nc, arith):
    """the top-up's shapes x gray and BGR x search 1, 2, 3, on the top-up's own block frames and on the ramp, with and without a weight plane"""
    import torch

    dev = _dev(torch)
    with rsdsfm.Solver(0, arith=arith) as s:
        k = 0
        for rows, cols in scases.SHAPES:
            for ch in (1, 3):
                for S in scases.SEARCHES:
                    image, mask, weight = scases.frame(rows, cols, ch, seed=S)
                    if k % 2:
                        image = cases.ramp_reference(rows, cols, ch, seed=k)[0]
                    curve, fallback, scale, ms, bms = cases.CURVES[k % len(cases.CURVES)]
                    weight = weight if k % 3 else None
                    k += 1
                    want = spec.denoise_spatial(image, mask, _lut(curve, fallback, scale, ms, bms), weight, 70, S)
                    p_i, p_m, p_n = Plane(image, 4, device=dev), Plane(mask, 4, device=dev), Plane(curve, 8, device=dev)
                    p_w = Plane(weight, 4, device=dev) if weight is not None else None
                    o_i, o_s, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev), fresh((3,), np.int64, 8, device=dev)
                    nc.denoise_spatial_curve_dev(s, p_i.ptr, p_m.ptr, p_w.ptr if p_w else None, ch, rows, cols, p_n.ptr, o_i.ptr, o_s.ptr, o_c.ptr, fallback, scale, ms, bms, 70, S)
                    s.synchronize()
                    assert np.array_equal(o_i.get(), want["image"]) and np.array_equal(o_s.get(), want["support"]) and o_c.get().tolist() == want["counts"], (rows, cols, ch, S)
                    assert p_i.unchanged() and p_m.unchanged() and p_n.unchanged() and (p_w is None or p_w.unchanged())


# (curve, fallback, scale, min_samples, band_min_samples, the strength of the existing call): flat curves, and curves whose row 8 has too few samples
FLAT = [(cases.flat_curve(700, 16), 0, 0, 0, 0, 12), (cases.flat_curve(700, 0), 30, 0, 0, 0, 1), (cases.flat_curve(700, 1023), 3, 0, 0, 0, 255),
        (cases.flat_curve(20, 9), 200, 40, 64, 16, 23), (cases.TOO_FEW, 33, 0, cases.MIN_SAMPLES, cases.BAND_MIN_SAMPLES, 33), (cases.RISING, 0, 0, 5000, 0, 12)]


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_a_flat_curve_and_too_few_samples_equal_the_existing_calls(rsdsfm, nc, arith):
    """the new kernels against the old: with a HAND-MADE flat curve in device memory the curve accumulate and the curve top-up are byte for byte
    rsdsfm_denoise_accumulate_dev and rsdsfm_denoise_spatial_dev at the strength the flat m asks for, and with row 8 below min_samples at the
    fallback"""
    import torch

    dev = _dev(torch)
    for curve, fallback, scale, ms, bms, h in FLAT:
        assert set(_lut(curve, fallback, scale, ms, bms).tolist()) == {h}
        assert nspec.noise_strength(int(curve[8, 0]), int(curve[8, 1]), scale, fallback or 12, ms) == h  # what the auto calls would form from row 8
    with rsdsfm.Solver(0, arith=arith) as s:
        for k, (rows, cols) in enumerate([(5, 5), (17, 65), (16, 131)]):
            for ch in (1, 3):
                ref, rmask = cases.ramp_reference(rows, cols, ch, seed=k)
                recs = dcases.records(ch)
                for L in (0, 1, 2, 3):
                    layers = dcases.layers(ref, rows, cols, ch, L, seed=k)
                    records = [list(recs.values())[(j + k) % 5] if (j + L) % 2 else None for j in range(L)]
                    for curve, fallback, scale, ms, bms, h in FLAT[(k + L) % 2::2]:
                        want = _accumulate_chain(torch, s, nc, ref, rmask, layers, records, None, h)
                        got = _accumulate_chain(torch, s, nc, ref, rmask, layers, records, curve, fallback, scale, ms, bms)
                        for key in ("image", "mask", "weight"):
                            assert np.array_equal(got[key], want[key]), (rows, cols, ch, L, h, key)
                        assert got["counts"] == want["counts"] and (want["cells"] is None or np.array_equal(got["cells"], want["cells"]))
        k = 0
        for rows, cols in [(2, 9), (17, 65), (33, 130)]:
            for ch in (1, 3):
                for S in scases.SEARCHES:
                    image, mask, weight = scases.frame(rows, cols, ch, seed=S)
                    curve, fallback, scale, ms, bms, h = FLAT[k % len(FLAT)]
                    weight = weight if k % 3 else None
                    k += 1
                    p_i, p_m, p_n = Plane(image, 4, device=dev), Plane(mask, 4, device=dev), Plane(curve, 8, device=dev)
                    p_w = Plane(weight, 4, device=dev) if weight is not None else None
                    got, want = [], []
                    for new, res in ((True, got), (False, want)):
                        o_i, o_s, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev), fresh((3,), np.int64, 8, device=dev)
                        if new:
                            nc.denoise_spatial_curve_dev(s, p_i.ptr, p_m.ptr, p_w.ptr if p_w else None, ch, rows, cols, p_n.ptr, o_i.ptr, o_s.ptr, o_c.ptr, fallback, scale, ms, bms, 70, S)
                        else:
                            s.denoise_spatial_dev(p_i.ptr, p_m.ptr, p_w.ptr if p_w else None, ch, rows, cols, o_i.ptr, o_s.ptr, o_c.ptr, h, 70, S)
                        s.synchronize()
                        res += [o_i.get(), o_s.get(), o_c.get().tolist()]
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (rows, cols, ch, S, h)


def test_curve_primitive_argument_errors(rsdsfm, nc):
    """the refusals the curve, the scale, min_samples and band_min_samples add; nothing is enqueued"""
    import torch

    dev = _dev(torch)
    rows, cols = 16, 64
    image, mask, weight = scases.frame(rows, cols, 3, seed=2)
    ref, rmask = dcases.reference(rows, cols, 3)
    (limg, lmask), = dcases.layers(ref, rows, cols, 3, 1)
    P = lambda a, al=4: Plane(a, al, device=dev)
    p_i, p_m, p_w, p_n, p_r, p_rm, p_l, p_lm = P(image), P(mask), P(weight), P(cases.RISING, 8), P(ref), P(rmask), P(limg), P(lmask)
    o_i, o_k, o_s, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev), fresh(
        (3,), np.int64, 8, device=dev)
    with rsdsfm.Solver(0) as s:
        def top_up(n=p_n.ptr, o=o_i.ptr, sp=o_s.ptr, cnt=o_c.ptr, h=0, scale=0, ms=0, bms=0, target=0, search=0):
            return nc.denoise_spatial_curve_dev(s, p_i.ptr, p_m.ptr, p_w.ptr, 3, rows, cols, n, o, sp, cnt, h, scale, ms, bms, target, search)

        def accumulate(n=p_n.ptr, o=o_i.ptr, cnt=o_c.ptr, h=0, scale=0, ms=0, bms=0, first=True, last=True):
            return nc.denoise_accumulate_curve_dev(s, p_r.ptr, p_rm.ptr, p_l.ptr, p_lm.ptr, 3, rows, cols, None, first, last, n, None, 0, 0, h, scale, ms, bms, o, o_k.ptr, o_s.ptr, cnt)

        for bad in (dict(n=0), dict(n=p_n.ptr + 4), dict(n=o_i.ptr), dict(cnt=p_n.ptr), dict(scale=256), dict(scale=-1), dict(ms=-1), dict(bms=-1), dict(h=256), dict(h=-1),
                    dict(target=256), dict(search=4), dict(o=p_i.ptr)):
            with pytest.raises(rsdsfm.RsdsfmError, match="denoise curve spatial: "):
                top_up(**bad)
        for bad in (dict(n=0), dict(n=p_n.ptr + 4), dict(o=p_n.ptr), dict(cnt=p_n.ptr), dict(scale=256), dict(scale=-1), dict(ms=-1), dict(bms=-1), dict(h=256), dict(h=-1),
                    dict(first=False), dict(o=p_r.ptr)):
            with pytest.raises(rsdsfm.RsdsfmError, match="denoise curve"):
                accumulate(**bad)
        s.synchronize()
        assert o_i.unchanged() and o_k.unchanged() and o_s.unchanged() and o_c.unchanged()
        top_up()
        s.synchronize()
        want = spec.denoise_spatial(image, mask, spec.strengths(cases.RISING), weight)
        assert np.array_equal(o_i.get(), want["image"]) and np.array_equal(o_s.get(), want["support"]) and o_c.get().tolist() == want["counts"]


# ---------------------------------------------------------------------------------------------------
# the frame call and the clip call
# ---------------------------------------------------------------------------------------------------
SPATIAL = dict(spatial=True, spatial_strength=120, target=60, search=3)
# the shift clip is a random texture: its |K * I| is large, so a small scale keeps the strengths off the clamp; the cases are small
CURVE_KW = dict(scale=1, min_samples=cases.MIN_SAMPLES, band_min_samples=cases.BAND_MIN_SAMPLES)


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
                curve=fresh((9, 4), np.uint64, 8, device=dev))


def _collect(o, top_up, with_optional=True):
    assert top_up or o["support"].unchanged()
    assert with_optional or (o["weight"].unchanged() and o["support"].unchanged() and o["counts"].unchanged() and o["curve"].unchanged())
    return dict(image=o["image"].get(), mask=o["mask"].get(), weight=o["weight"].get() if with_optional else None, support=o["support"].get() if top_up and with_optional else None,
                counts=o["counts"].get().tolist() if with_optional else None, curve=o["curve"].get().tolist() if with_optional else None)


def _same_frame(got, want, name=""):
    for k in ("image", "mask", "weight", "support"):
        assert got[k] is None or np.array_equal(got[k], want[k]), (name, k)
    for k in ("counts", "curve"):
        assert got[k] is None or list(got[k]) == list(want[k]), (name, k, got[k], want[k])


def _frame(torch, s, nc, case, d=None, q=None, top_up=False, with_optional=True, curve_kw=CURVE_KW):
    """one rsdsfm_denoise_curve_frame_dev of frame q of a case into guarded, never preset outputs"""
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = d or _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case, q)
    o = _outputs(dev, case)
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    opt = lambda k: o[k].ptr if with_optional else None
    nc.denoise_curve_frame_dev(s, pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, o["image"].ptr, o["mask"].ptr, opt("weight"),
                               opt("support") if top_up else None, opt("counts"), opt("curve"), **_frame_kw(case), **curve_kw, **(SPATIAL if top_up else {}))
    s.synchronize()
    for t, a in zip(d["frames"], case["frames"]):
        assert np.array_equal(t.cpu().numpy(), a)
    return _collect(o, top_up, with_optional)


def _public_calls(torch, s, nc, case, q=None, top_up=False, curve_kw=CURVE_KW):
    """what the frame call promises to equal, public calls one after another on planes of the test's own: the rendered reference planes (the
    existing frame call on the own frame alone gives them as its image and mask), rsdsfm_noise_curve_dev on them, then per neighbour
    rsdsfm_denoise_accumulate_curve_dev on the layer and the record the denoise's definition renders (tests/test_gpu_denoise.py holds the
    library's renders to it byte for byte), then rsdsfm_denoise_spatial_curve_dev"""
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case, q)
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    ref, rmask = fresh(case["frames"][0].shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev)
    s.denoise_frame_dev(pick("frames")[:1], ch, pick("maps")[:1], pick("Rs")[:1], pick("ts")[:1], case["K"], rows, cols, M[:1], m[:1], ref.ptr, rmask.ptr, **_frame_kw(case))
    hist, cur = fresh(HIST, np.uint32, 4, device=dev), fresh((9, 4), np.uint64, 8, device=dev)
    nc.noise_curve_dev(s, ref.ptr, rmask.ptr, ch, rows, cols, hist.ptr, cur.ptr)
    s.synchronize()
    want = dcases.run_spec(case, q)
    assert np.array_equal(ref.get(), want["ref"][0]) and np.array_equal(rmask.get(), want["ref"][1])
    curve = cur.get()
    assert curve.tolist() == spec.noise_curve(ref.get(), rmask.get())["curve"].tolist()
    kw = dict(strength=case["strength"], scale=curve_kw.get("scale", 0), min_samples=curve_kw.get("min_samples", 0), band_min_samples=curve_kw.get("band_min_samples", 0))
    acc = _accumulate_chain(torch, s, nc, ref.get(), rmask.get(), want["layers"], list(want["records"]), curve, **kw)
    out = dict(image=acc["image"], mask=acc["mask"], weight=acc["weight"], support=None, counts=acc["counts"] + [0, 0, 0], curve=curve.tolist(),
               lut=nc.noise_curve_strengths(curve, kw["scale"], kw["strength"], kw["min_samples"], kw["band_min_samples"]))
    if top_up:
        P = lambda a, al=4: Plane(a, al, device=dev)
        p_i, p_m, p_w, p_n = P(acc["image"]), P(acc["mask"]), P(acc["weight"]), P(curve, 8)
        o_i, o_s, o_c = fresh(acc["image"].shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev), fresh((3,), np.int64, 8, device=dev)
        nc.denoise_spatial_curve_dev(s, p_i.ptr, p_m.ptr, p_w.ptr, ch, rows, cols, p_n.ptr, o_i.ptr, o_s.ptr, o_c.ptr, SPATIAL["spatial_strength"], kw["scale"], kw["min_samples"],
                                     kw["band_min_samples"], SPATIAL["target"], SPATIAL["search"])
        s.synchronize()
        out.update(image=o_i.get(), support=o_s.get(), counts=acc["counts"] + o_c.get().tolist())
    return out


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_frame_call_equals_the_public_calls(rsdsfm, nc, arith):
    """denoise_cases' noisy shift clip, BGR and gray, from its middle (four neighbours) and from its first frame (one-sided), with and without
    the top-up, with and without the optional outputs; the defaults (1024 samples or the fallback) once"""
    import torch

    tables = set()
    with rsdsfm.Solver(0, arith=arith) as s:
        for case, q in ((dcases.shift_clip(0, 3), None), (dcases.shift_clip(1, 1), 0)):
            rows, cols = case["depths"][0].shape
            nsrc = len(dcases.sources_and_poses(case, q)[0])
            for top_up in (False, True):
                want = _public_calls(torch, s, nc, case, q, top_up)
                tables.add(len(set(want["lut"].tolist())))
                _same_frame(_frame(torch, s, nc, case, q=q, top_up=top_up), want, (case["name"], top_up))
                _same_frame(_frame(torch, s, nc, case, q=q, top_up=top_up, with_optional=False), want, (case["name"], top_up, "bare"))
                assert nc.denoise_curve_frame_launches(rows, cols, nsrc, top_up) == rsdsfm.denoise_launches(rows, cols, nsrc) + 2 + int(top_up)
        case = dcases.shift_clip(0, 3)
        _same_frame(_frame(torch, s, nc, case, curve_kw=dict()), _public_calls(torch, s, nc, case, curve_kw=dict()), "defaults")
    assert max(tables) > 1  # a table with more than one strength was used


def test_frame_argument_errors(rsdsfm, nc):
    """a refused frame call enqueues nothing: the outputs keep their guard bytes"""
    import torch

    dev = _dev(torch)
    case = dcases.shift_clip(0, 3)
    rows, cols = case["depths"][0].shape
    d = _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case)
    o = _outputs(dev, case)
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    with rsdsfm.Solver(0) as s:
        def call(images=pick("frames"), maps=pick("maps"), M=M, m=m, i=o["image"].ptr, k=o["mask"].ptr, w=o["weight"].ptr, sp=o["support"].ptr, cnt=o["counts"].ptr,
                 cv=o["curve"].ptr, ch=3, spatial=True, **kw):
            return nc.denoise_curve_frame_dev(s, images, ch, maps, pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, i, k, w, sp, cnt, cv, spatial=spatial, **kw)

        bad_M = M.copy()
        bad_M[1, 0, 0] = np.nan
        params, sparams, cparams = rsdsfm.DenoiseParams(), rsdsfm.DenoiseSpatialParams(), nc.NoiseCurveParams()
        params.struct_bytes, sparams.struct_bytes, cparams.struct_bytes = 40, 28, 40
        bads = (dict(images=[0] + pick("frames")[1:]), dict(maps=pick("maps")[:1] + [0] * (len(src) - 1)), dict(images=[]), dict(M=bad_M), dict(i=0), dict(k=0),
                dict(i=o["mask"].ptr), dict(w=o["image"].ptr), dict(sp=o["image"].ptr), dict(i=o["image"].ptr + 1), dict(cnt=o["counts"].ptr + 4), dict(i=pick("frames")[1]),
                dict(ch=2), dict(strength=256), dict(window=(0, 0, rows + 1, cols)), dict(params=params), dict(spatial_params=sparams), dict(curve_params=cparams),
                dict(search=4), dict(spatial=False), dict(cv=o["curve"].ptr + 4), dict(cv=o["counts"].ptr), dict(cv=o["image"].ptr), dict(cv=pick("frames")[0]),
                dict(cv=pick("maps")[1]), dict(quantile_q8=257), dict(scale=256), dict(min_samples=-1), dict(band_min_samples=-1))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        assert all(p.unchanged() for p in o.values())
        call(strength=case["strength"], **CURVE_KW, **SPATIAL)
        s.synchronize()
        _same_frame(_collect(o, True), _public_calls(torch, s, nc, case, top_up=True))


def _video(torch, s, nc, case, top_up, want_counts=True, want_curves=True, with_optional=True):
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    ns = len(case["depths"])
    d = _clip(torch, dev, case)
    outs = [_outputs(dev, case) for _ in range(ns)]
    ptrs = lambda a: [x.data_ptr() for x in a]
    col = lambda k: [o[k].ptr for o in outs]
    r = nc.denoise_curve_video_dev(s, ptrs(d["frames"]), rows, cols, ch, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"],
                                   case["c_path"], case["scales"], col("image"), col("mask"), col("weight") if with_optional else None,
                                   col("support") if with_optional and top_up else None, want_counts=want_counts, want_curves=want_curves, radius=case["radius"],
                                   **_frame_kw(case), **CURVE_KW, **(SPATIAL if top_up else {}))
    s.synchronize()
    got = []
    for q, o in enumerate(outs):
        assert o["counts"].unchanged() and o["curve"].unchanged() and (top_up and with_optional or o["support"].unchanged()) and (with_optional or o["weight"].unchanged())
        got.append(dict(image=o["image"].get(), mask=o["mask"].get(), weight=o["weight"].get() if with_optional else None,
                        support=o["support"].get() if top_up and with_optional else None, counts=r["counts"][q].tolist() if want_counts else None,
                        curve=r["curves"][q].tolist() if want_curves else None))
    assert set(r) == ({"counts"} if want_counts else set()) | ({"curves"} if want_curves else set())
    return got, d, outs


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_clip_call_equals_the_frame_calls(rsdsfm, nc, arith):
    """the shift clip's five frames at radius 2 (one-sided neighbours at the ends), BGR with and gray without the top-up: every frame of the clip
    call is the frame call's, counters and curves included; with neither host array the call only enqueues; a refused call enqueues nothing"""
    import torch

    with rsdsfm.Solver(0, arith=arith) as s:
        for case, top_up in ((dcases.shift_clip(0, 3), True), (dcases.shift_clip(1, 1), False)):
            got, d, _ = _video(torch, s, nc, case, top_up)
            for q in range(len(case["depths"])):
                _same_frame(got[q], _frame(torch, s, nc, case, d, q, top_up), (case["name"], q))
        case = dcases.shift_clip(0, 3)
        full, _, _ = _video(torch, s, nc, case, True)
        for kw in (dict(want_counts=False), dict(want_curves=False), dict(want_counts=False, want_curves=False, with_optional=False)):
            got, _, _ = _video(torch, s, nc, case, True, **kw)
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
            return nc.denoise_curve_video_dev(s, ptrs(d["frames"]), rows, cols, 3, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"],
                                              case["c_path"], scales, i or [o["image"].ptr for o in outs], [o["mask"].ptr for o in outs], None, sp, **kw)

        for bad in (dict(scales=bad_scales), dict(radius=8), dict(strength=300), dict(spatial=True, search=4), dict(scale=256), dict(quantile_q8=300), dict(min_samples=-1),
                    dict(band_min_samples=-1), dict(i=[outs[0]["image"].ptr] * (ns - 1) + [0]), dict(sp=[o["support"].ptr for o in outs]),
                    dict(i=[outs[0]["image"].ptr] * (ns - 1) + [d["frames"][1].data_ptr()])):
            with pytest.raises(rsdsfm.RsdsfmError, match="denoise curve video|rsdsfm_"):
                call(**bad)
        s.synchronize()
        assert all(p.unchanged() for o in outs for p in o.values())


# ---------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------
def test_evaluate_real_sequence_with_the_noise_curve(rsdsfm, nc, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, denoise=(K, "curve"[, spatial])) on a small clip under signal-dependent sensor noise
    (render_sequence(noise=(2, 20))) adds exactly denoise_curve to the keys of the same call with an integer strength and eleven columns to
    denoise.csv; with "auto" every key and file is what it is without this module; any other string stays a ValueError"""
    from test_gpu_stabilize_search import TRIALS

    rows, cols, gamma = 16, 64, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    sc = 4.0 / np.abs(f0).max()
    frames, _, _ = rsdsfm.synth.render_sequence(3, rows, cols, K, v * sc, w * sc, k, gamma, seed=21, speeds=(1.0, 1.3), noise=(2, 20))
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=[3, 8], stabilize=True, smooth_sigma=1.0)
    n = len(frames) - 1
    with rsdsfm.Solver(0) as s:
        curved = ev(s, frames, denoise=(2, "curve"), out_dir=str(tmp_path / "curve"), **kw)
        topped = ev(s, frames, denoise=(2, "curve", True), **kw)
        plain = ev(s, frames, denoise=(2, 30), out_dir=str(tmp_path / "plain"), **kw)
        auto = ev(s, frames, denoise=(2, "auto"), out_dir=str(tmp_path / "auto"), **kw)
        assert set(curved) == set(plain) | {"denoise_curve"} and set(topped) == set(curved) | {"denoise_support", "denoise_spatial_counts"}
        assert set(auto) == set(plain) | {"denoise_noise"}
        curve = curved["denoise_curve"]
        assert curve.shape == (n, 9, 4) and curve.dtype == np.int64 and np.array_equal(curve, topped["denoise_curve"]) and (curve[:, 8, 0] > 0).all()
        assert np.array_equal(curve[:, 8, :3], auto["denoise_noise"][:, :3])  # row 8 is the noise level's record
        assert (curve[:, :8, 0].sum(axis=1) == curve[:, 8, 0]).all()
        for key in plain:
            if key not in ("pairs", "path_smoothed", "links", "stab_denoised", "denoise_masks", "denoise_weights", "denoise_counts"):
                assert np.asarray(curved[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
        with pytest.raises(ValueError):
            ev(s, frames, denoise=(2, "strong"), **kw)
    lines = open(str(tmp_path / "curve" / "denoise.csv")).read().split()
    assert lines[0] == "pair,unset,own_only,averaged,mean_weight," + ",".join("noise_m%d" % b for b in range(8)) + ",noise_m,strength_min,strength_max" and len(lines) == 1 + n
    lut = nc.noise_curve_strengths(curve[0].astype(np.uint64))
    assert lines[1].split(",")[5:] == [str(int(x)) for x in curve[0, :, 1]] + [str(int(lut.min())), str(int(lut.max()))]
    assert open(str(tmp_path / "auto" / "denoise.csv")).read().split()[0] == "pair,unset,own_only,averaged,mean_weight,noise_m,sigma,strength"
    assert open(str(tmp_path / "plain" / "denoise.csv")).read().split()[0] == "pair,unset,own_only,averaged,mean_weight"
    assert set(os.listdir(str(tmp_path / "curve"))) == set(os.listdir(str(tmp_path / "plain"))) == set(os.listdir(str(tmp_path / "auto")))
