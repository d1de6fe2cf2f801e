"""GPU: the sharpen stage (include/rsdsfm_sharpen.h) bit for bit against its definition (tests/sharpen_spec_numpy.py) in both library builds --
the primitive at the shapes where its 16 x 64 tile, its halo of 2, its byte paths and frames smaller than the halo can go wrong, with and without
the counters; the curve form against the definition under hand-made curves, and against the fixed form under a flat curve and under a curve
with too few samples; the frame call against the two public calls made one after another; the clip call against the frame calls;
evaluate_real_sequence(sharpen=...); and the refusals of every call.  Every plane sits at the minimum alignment the header admits (4 bytes and
not 8; the curves and counters 8 and not 16) between guard bytes (tests/guarded_planes.py); the outputs are never preset and the inputs are
verified unchanged."""
import os

import numpy as np
import pytest

import noise_curve_cases as ccases
import noise_curve_spec_numpy as cspec
import noise_spec_numpy as nspec
import sharpen_cases as cases
import sharpen_spec_numpy as spec
from guarded_planes import Plane, fresh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sh():
    import rsdsfm_sharpen

    return rsdsfm_sharpen


@pytest.fixture(scope="module")
def nc():
    import rsdsfm_noise_curve

    return rsdsfm_noise_curve


def _dev(torch):
    return torch.device("cuda", 0)


def _ch(image):
    return 1 if image.ndim == 2 else 3


# ---------------------------------------------------------------------------------------------------
# the primitive
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_primitive_equals_the_definition(rsdsfm, sh, arith):
    """every shape of sharpen_cases.SHAPES x one and three channels x every kind, the parameter sets and the strength cycling: every output byte
    and the four counters are the definition's; without the counters the bytes are the same"""
    import torch

    dev = _dev(torch)
    with rsdsfm.Solver(0, arith=arith) as s:
        every = cases.primitive_cases()
        assert {c["image"].shape[:2] for c in every} == set(cases.SHAPES) and {c["kind"] for c in every} == set(cases.KINDS)
        for k, case in enumerate(every):
            image, mask = case["image"], case["mask"]
            rows, cols = mask.shape
            want = cases.run_spec(case)
            p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
            o_i, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((4,), np.int64, 8, device=dev)
            with_counts = k % 3 != 2
            sh.sharpen_dev(s, p_i.ptr, p_m.ptr, _ch(image), rows, cols, o_i.ptr, o_c.ptr if with_counts else None, case["amount_q4"], case["coring_q4"], case["overshoot"],
                           case["strength"])
            s.synchronize()
            assert p_i.unchanged() and p_m.unchanged()
            assert np.array_equal(o_i.get(), want["image"]), case["name"]
            assert o_c.get().tolist() == want["counts"] if with_counts else o_c.unchanged(), (case["name"], o_c.get(), want["counts"])
        assert sh.sharpen_launches() == 1 and sh.sharpen_frame_launches() == 3
        assert sh.sharpen_default_params() == dict(amount_q4=16, coring_q4=8, overshoot=0, strength=12)


def test_primitive_argument_errors(rsdsfm, sh):
    """every refusal is RSDSFM_ERR_INVALID with a "sharpen: " message and enqueues nothing: the outputs keep their guard bytes; after a refused
    call the same call without the fault goes through"""
    import torch

    dev = _dev(torch)
    rows, cols = 16, 64
    image, mask = cases.frame(rows, cols, 3, "noisy", seed=2)
    p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
    o_i, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((4,), np.int64, 8, device=dev)
    with rsdsfm.Solver(0) as s:
        def call(i=p_i.ptr, m=p_m.ptr, ch=3, r=rows, c=cols, o=o_i.ptr, cnt=o_c.ptr, a=16, co=8, ov=0, h=0):
            return sh.sharpen_dev(s, i, m, ch, r, c, o, cnt, a, co, ov, h)

        bads = (dict(i=0), dict(m=0), dict(o=0), dict(i=p_i.ptr + 1), dict(m=p_m.ptr + 2), dict(o=o_i.ptr + 2), dict(cnt=o_c.ptr + 4), dict(o=p_i.ptr), dict(o=p_m.ptr),
                dict(cnt=o_i.ptr), dict(ch=2), dict(ch=4), dict(r=1), dict(c=1), dict(r=16385), dict(c=16385), dict(a=-1), dict(a=65), dict(co=-1),
                dict(co=65), dict(ov=-1), dict(ov=256), dict(h=-1), dict(h=256))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError, match="sharpen: "):
                call(**bad)
        s.synchronize()
        assert o_i.unchanged() and o_c.unchanged()  # nothing was enqueued
        call()
        s.synchronize()
        want = spec.sharpen(image, mask)
        assert np.array_equal(o_i.get(), want["image"]) and o_c.get().tolist() == want["counts"] and p_i.unchanged() and p_m.unchanged()


# ---------------------------------------------------------------------------------------------------
# the curve form
# ---------------------------------------------------------------------------------------------------
def _lut(curve, fallback, scale, ms, bms):
    return cspec.strengths(curve, scale, fallback or 12, ms, bms)


CURVE_SHAPES = [(5, 5), (17, 65), (16, 131), (35, 67)]


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_curve_form_equals_the_definition(rsdsfm, sh, arith):
    """noise_curve_cases.CURVES (every band valid, invalid bands, no band valid, too few samples, a caller's scale) on ramp_reference inputs,
    which walk through every level: every byte and the counters are the definition's at the table's strength per pixel"""
    import torch

    dev = _dev(torch)
    differs = 0
    with rsdsfm.Solver(0, arith=arith) as s:
        k = 0
        for rows, cols in CURVE_SHAPES:
            for ch in (1, 3):
                for curve, fallback, scale, ms, bms in ccases.CURVES:
                    image, mask = ccases.ramp_reference(rows, cols, ch, seed=k)
                    amount, coring, overshoot = cases.PARAMS[k % len(cases.PARAMS)]
                    k += 1
                    lut = _lut(curve, fallback, scale, ms, bms)
                    want = spec.sharpen(image, mask, amount, coring, overshoot, fallback or 12, lut)
                    p_i, p_m, p_n = Plane(image, 4, device=dev), Plane(mask, 4, device=dev), Plane(curve, 8, device=dev)
                    o_i, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((4,), np.int64, 8, device=dev)
                    sh.sharpen_curve_dev(s, p_i.ptr, p_m.ptr, ch, rows, cols, p_n.ptr, o_i.ptr, o_c.ptr, amount, coring, overshoot, fallback, scale, ms, bms)
                    s.synchronize()
                    assert np.array_equal(o_i.get(), want["image"]) and o_c.get().tolist() == want["counts"], (rows, cols, ch, k)
                    assert p_i.unchanged() and p_m.unchanged() and p_n.unchanged()
                    if len(set(lut.tolist())) > 1:
                        flat = spec.sharpen(image, mask, amount, coring, overshoot, int(np.median(lut)))
                        differs += int(not np.array_equal(flat["image"], want["image"]))
    assert differs > 0  # the strength per pixel matters on these inputs


# (curve, fallback, scale, min_samples, band_min_samples, the strength of the fixed call): flat curves, and curves whose row 8 has too few samples
FLAT = [(ccases.flat_curve(700, 16), 0, 0, 0, 0, 12), (ccases.flat_curve(700, 0), 30, 0, 0, 0, 1), (ccases.flat_curve(700, 1023), 3, 0, 0, 0, 255),
        (ccases.flat_curve(20, 9), 200, 40, 64, 16, 23), (ccases.TOO_FEW, 33, 0, ccases.MIN_SAMPLES, ccases.BAND_MIN_SAMPLES, 33), (ccases.RISING, 0, 0, 5000, 0, 12)]


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_a_flat_curve_and_too_few_samples_equal_the_fixed_form(rsdsfm, sh, arith):
    """with a HAND-MADE flat curve in device memory rsdsfm_sharpen_curve_dev is byte for byte rsdsfm_sharpen_dev at the strength the flat m asks
    for (rsdsfm_noise_strength), and with row 8 below min_samples at the fallback"""
    import torch

    dev = _dev(torch)
    for curve, fallback, scale, ms, bms, h in FLAT:
        assert set(_lut(curve, fallback, scale, ms, bms).tolist()) == {h}
        assert nspec.noise_strength(int(curve[8, 0]), int(curve[8, 1]), scale, fallback or 12, ms) == h
    with rsdsfm.Solver(0, arith=arith) as s:
        k = 0
        for rows, cols in [(2, 9), (17, 65), (33, 130)]:
            for ch in (1, 3):
                for kind in ("noisy", "holes", "step"):
                    image, mask = cases.frame(rows, cols, ch, kind, seed=k)
                    curve, fallback, scale, ms, bms, h = FLAT[k % len(FLAT)]
                    amount, coring, overshoot = [p for p in cases.PARAMS if p[0] and p[1]][k % 3]
                    k += 1
                    p_i, p_m, p_n = Plane(image, 4, device=dev), Plane(mask, 4, device=dev), Plane(curve, 8, device=dev)
                    got, want = [], []
                    for new, res in ((True, got), (False, want)):
                        o_i, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((4,), np.int64, 8, device=dev)
                        if new:
                            sh.sharpen_curve_dev(s, p_i.ptr, p_m.ptr, ch, rows, cols, p_n.ptr, o_i.ptr, o_c.ptr, amount, coring, overshoot, fallback, scale, ms, bms)
                        else:
                            sh.sharpen_dev(s, p_i.ptr, p_m.ptr, ch, rows, cols, o_i.ptr, o_c.ptr, amount, coring, overshoot, h)
                        s.synchronize()
                        res += [o_i.get(), o_c.get().tolist()]
                    assert np.array_equal(got[0], want[0]) and got[1] == want[1], (rows, cols, ch, kind, h)
                    assert np.array_equal(want[0], spec.sharpen(image, mask, amount, coring, overshoot, h)["image"])


def test_curve_primitive_argument_errors(rsdsfm, sh):
    """the fixed form's refusals and those the curve, the scale, min_samples and band_min_samples add, with the "sharpen curve: " prefix; nothing
    is enqueued"""
    import torch

    dev = _dev(torch)
    rows, cols = 16, 64
    image, mask = ccases.ramp_reference(rows, cols, 3, seed=1)
    p_i, p_m, p_n = Plane(image, 4, device=dev), Plane(mask, 4, device=dev), Plane(ccases.RISING, 8, device=dev)
    o_i, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((4,), np.int64, 8, device=dev)
    with rsdsfm.Solver(0) as s:
        def call(i=p_i.ptr, m=p_m.ptr, ch=3, r=rows, c=cols, n=p_n.ptr, o=o_i.ptr, cnt=o_c.ptr, a=16, co=8, ov=0, h=0, scale=0, ms=0, bms=0):
            return sh.sharpen_curve_dev(s, i, m, ch, r, c, n, o, cnt, a, co, ov, h, scale, ms, bms)

        bads = (dict(i=0), dict(m=0), dict(o=0), dict(n=0), dict(n=p_n.ptr + 4), dict(n=o_c.ptr), dict(cnt=p_n.ptr), dict(i=p_i.ptr + 2), dict(o=o_i.ptr + 1),
                dict(cnt=o_c.ptr + 4), dict(o=p_i.ptr), dict(o=p_m.ptr), dict(ch=2), dict(r=1), dict(c=16385), dict(a=65), dict(co=-1), dict(ov=256), dict(h=256), dict(h=-1),
                dict(scale=256), dict(scale=-1), dict(ms=-1), dict(bms=-1))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError, match="sharpen curve: "):
                call(**bad)
        s.synchronize()
        assert o_i.unchanged() and o_c.unchanged()
        call()
        s.synchronize()
        want = spec.sharpen(image, mask, lut=cspec.strengths(ccases.RISING))
        assert np.array_equal(o_i.get(), want["image"]) and o_c.get().tolist() == want["counts"]


# ---------------------------------------------------------------------------------------------------
# the frame call and the clip call
# ---------------------------------------------------------------------------------------------------
# the cases are small: the defaults (1024 and 256 samples) are more than some of them have
CURVE_KW = dict(min_samples=ccases.MIN_SAMPLES, band_min_samples=ccases.BAND_MIN_SAMPLES)
FRAME_KW = dict(amount_q4=32, coring_q4=8, overshoot=8, strength=20, quantile_q8=140, scale=10)


def _frame_inputs(ch, seed=0, shape=(33, 130)):
    """the noise curve's ramp under noise that grows with the level: a table with more than one strength"""
    image, mask = ccases.frame(shape[0], shape[1], ch, "ramp", seed=seed)
    mask[3:6, 10:20] = 0
    return image, mask


def _frame(torch, s, sh, image, mask, with_curve=True, with_counts=True, **kw):
    dev = _dev(torch)
    rows, cols = mask.shape
    p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
    o_i, o_c, o_n = fresh(image.shape, np.uint8, 4, device=dev), fresh((4,), np.int64, 8, device=dev), fresh((9, 4), np.uint64, 8, device=dev)
    sh.sharpen_frame_dev(s, p_i.ptr, p_m.ptr, _ch(image), rows, cols, o_i.ptr, o_c.ptr if with_counts else None, o_n.ptr if with_curve else None, **kw)
    s.synchronize()
    assert p_i.unchanged() and p_m.unchanged() and (with_curve or o_n.unchanged()) and (with_counts or o_c.unchanged())
    return dict(image=o_i.get(), counts=o_c.get().tolist() if with_counts else None, curve=o_n.get().tolist() if with_curve else None)


def _public_calls(torch, s, sh, nc, image, mask, amount_q4=16, coring_q4=8, overshoot=0, strength=0, quantile_q8=0, scale=0, min_samples=0, band_min_samples=0):
    """what the frame call promises to equal: rsdsfm_noise_curve_dev, then rsdsfm_sharpen_curve_dev on its curve, on planes of the test's own"""
    dev = _dev(torch)
    rows, cols = mask.shape
    p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
    hist, cur = fresh((cspec.BANDS, cspec.BINS), np.uint32, 4, device=dev), fresh((9, 4), np.uint64, 8, device=dev)
    o_i, o_c = fresh(image.shape, np.uint8, 4, device=dev), fresh((4,), np.int64, 8, device=dev)
    nc.noise_curve_dev(s, p_i.ptr, p_m.ptr, _ch(image), rows, cols, hist.ptr, cur.ptr, quantile_q8)
    sh.sharpen_curve_dev(s, p_i.ptr, p_m.ptr, _ch(image), rows, cols, cur.ptr, o_i.ptr, o_c.ptr, amount_q4, coring_q4, overshoot, strength, scale, min_samples, band_min_samples)
    s.synchronize()
    curve = cur.get()
    want = spec.sharpen_frame(image, mask, amount_q4, coring_q4, overshoot, strength or 12, quantile_q8, scale, min_samples, band_min_samples)
    assert curve.tolist() == want["curve"].tolist() and np.array_equal(o_i.get(), want["image"]) and o_c.get().tolist() == want["counts"]  # and both are the definition's
    return dict(image=o_i.get(), counts=o_c.get().tolist(), curve=curve.tolist(), lut=want["lut"])


def _same_frame(got, want, name=""):
    assert np.array_equal(got["image"], want["image"]), name
    for k in ("counts", "curve"):
        assert got[k] is None or list(got[k]) == list(want[k]), (name, k, got[k], want[k])


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_frame_call_equals_the_public_calls(rsdsfm, sh, nc, arith):
    """gray and BGR, with the curve returned and with it left in the workspace, with and without the counters, a caller's parameters and the
    defaults (1024 samples or the fallback); a second size on the same context (the workspace follows)"""
    import torch

    tables = set()
    with rsdsfm.Solver(0, arith=arith) as s:
        for ch in (1, 3):
            image, mask = _frame_inputs(ch, seed=ch)
            for kw in (dict(CURVE_KW), dict(FRAME_KW, **CURVE_KW), dict()):
                want = _public_calls(torch, s, sh, nc, image, mask, **kw)
                tables.add(len(set(want["lut"].tolist())))
                _same_frame(_frame(torch, s, sh, image, mask, **kw), want, (ch, kw))
                _same_frame(_frame(torch, s, sh, image, mask, with_curve=False, **kw), want, (ch, kw, "workspace curve"))
                _same_frame(_frame(torch, s, sh, image, mask, with_curve=False, with_counts=False, **kw), want, (ch, kw, "bare"))
        image, mask = _frame_inputs(3, seed=5, shape=(17, 65))
        _same_frame(_frame(torch, s, sh, image, mask, **CURVE_KW), _public_calls(torch, s, sh, nc, image, mask, **CURVE_KW), "second size")
        r = sh.sharpen(s, image, mask, **CURVE_KW)  # the host convenience
        want = spec.sharpen_frame(image, mask, **CURVE_KW)
        assert np.array_equal(r["image"], want["image"]) and r["counts"] == want["counts"] and r["curve"].tolist() == want["curve"].tolist()
        assert np.array_equal(r["lut"], want["lut"])
        assert sh.sharpen_frame_launches() == nc.noise_curve_launches() + sh.sharpen_launches()
    assert max(tables) > 1  # a table with more than one strength was used


def test_frame_argument_errors(rsdsfm, sh):
    """a refused frame call enqueues nothing: the outputs keep their guard bytes; in-place, non-zero reserved words and a wrong struct_bytes are
    among the refusals"""
    import torch

    dev = _dev(torch)
    image, mask = _frame_inputs(3, seed=2, shape=(16, 64))
    rows, cols = mask.shape
    p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
    o_i, o_c, o_n = fresh(image.shape, np.uint8, 4, device=dev), fresh((4,), np.int64, 8, device=dev), fresh((9, 4), np.uint64, 8, device=dev)
    with rsdsfm.Solver(0) as s:
        def call(i=p_i.ptr, m=p_m.ptr, ch=3, r=rows, c=cols, o=o_i.ptr, cnt=o_c.ptr, cv=o_n.ptr, **kw):
            return sh.sharpen_frame_dev(s, i, m, ch, r, c, o, cnt, cv, **kw)

        short, reserved, cshort = sh.SharpenParams(16, 8, 0, 12, 28), sh.SharpenParams(16, 8, 0, 12, 32), sh.NoiseCurveParams()
        reserved.reserved[1] = 1
        cshort.struct_bytes = 40
        bads = (dict(i=0), dict(m=0), dict(o=0), dict(i=p_i.ptr + 1), dict(o=o_i.ptr + 2), dict(cnt=o_c.ptr + 4), dict(cv=o_n.ptr + 4), dict(o=p_i.ptr), dict(o=p_m.ptr),
                dict(cv=o_c.ptr), dict(cv=o_i.ptr), dict(cv=p_i.ptr), dict(ch=2), dict(r=1), dict(c=16385), dict(amount_q4=65), dict(amount_q4=-1), dict(coring_q4=65),
                dict(overshoot=256), dict(strength=256), dict(params=short), dict(params=reserved), dict(curve_params=cshort), dict(quantile_q8=257), dict(scale=256),
                dict(min_samples=-1), dict(band_min_samples=-1))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError, match="sharpen frame: "):
                call(**bad)
        s.synchronize()
        assert o_i.unchanged() and o_c.unchanged() and o_n.unchanged()
        call(**CURVE_KW)
        s.synchronize()
        want = spec.sharpen_frame(image, mask, **CURVE_KW)
        assert np.array_equal(o_i.get(), want["image"]) and o_c.get().tolist() == want["counts"] and o_n.get().tolist() == want["curve"].tolist()


def _video(torch, s, sh, clip, want_counts=True, want_curves=True, **kw):
    dev = _dev(torch)
    rows, cols = clip[0][1].shape
    p = [(Plane(i, 4, device=dev), Plane(m, 4, device=dev)) for i, m in clip]
    outs = [fresh(i.shape, np.uint8, 4, device=dev) for i, _ in clip]
    r = sh.sharpen_video_dev(s, [a.ptr for a, _ in p], [b.ptr for _, b in p], _ch(clip[0][0]), rows, cols, [o.ptr for o in outs], want_counts, want_curves, **kw)
    s.synchronize()
    assert all(a.unchanged() and b.unchanged() for a, b in p)
    assert set(r) == ({"counts"} if want_counts else set()) | ({"curves"} if want_curves else set())
    return [dict(image=o.get(), counts=r["counts"][q].tolist() if want_counts else None, curve=r["curves"][q].tolist() if want_curves else None) for q, o in enumerate(outs)]


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_clip_call_equals_the_frame_calls(rsdsfm, sh, arith):
    """three frames, BGR and gray: every frame of the clip call is the frame call's, counters and curves included; with one host array or none
    the bytes are the same; a refused call enqueues nothing"""
    import torch

    dev = _dev(torch)
    with rsdsfm.Solver(0, arith=arith) as s:
        for ch in (3, 1):
            clip = [_frame_inputs(ch, seed=10 + q, shape=(18, 66)) for q in range(3)]
            kw = dict(FRAME_KW, **CURVE_KW)
            full = _video(torch, s, sh, clip, **kw)
            for q, (image, mask) in enumerate(clip):
                _same_frame(full[q], _frame(torch, s, sh, image, mask, **kw), (ch, q))
            for flags in (dict(want_counts=False), dict(want_curves=False), dict(want_counts=False, want_curves=False)):
                got = _video(torch, s, sh, clip, **flags, **kw)
                for q in range(len(clip)):
                    _same_frame(got[q], full[q], (ch, q, flags))
        clip = [_frame_inputs(3, seed=20 + q, shape=(16, 64)) for q in range(3)]
        p = [(Plane(i, 4, device=dev), Plane(m, 4, device=dev)) for i, m in clip]
        outs = [fresh(i.shape, np.uint8, 4, device=dev) for i, _ in clip]
        I, M, O = [a.ptr for a, _ in p], [b.ptr for _, b in p], [o.ptr for o in outs]

        def call(i=I, m=M, o=O, ch=3, r=16, c=64, **kw):
            return sh.sharpen_video_dev(s, i, m, ch, r, c, o, **kw)

        reserved = sh.SharpenParams(16, 8, 0, 12, 32)
        reserved.reserved[0] = 7
        for bad in (dict(i=I[:2] + [0]), dict(m=[0] + M[1:]), dict(o=O[:2] + [0]), dict(o=O[:2] + [I[0]]), dict(o=O[:2] + [M[1]]), dict(o=[O[0], O[1], O[0]]),
                    dict(o=[O[0], O[1], O[2] + 1]), dict(ch=2), dict(r=1), dict(amount_q4=65), dict(params=reserved), dict(params=sh.SharpenParams(16, 8, 0, 12, 31)),
                    dict(scale=256), dict(quantile_q8=300)):
            with pytest.raises(rsdsfm.RsdsfmError, match="sharpen video: "):
                call(**bad)
        s.synchronize()
        assert all(o.unchanged() for o in outs)


# ---------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------
def test_evaluate_real_sequence_with_sharpen(rsdsfm, sh, nc, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, sharpen=True) on the small clip of the noise curve's evaluate test adds exactly the four
    sharpen keys, sharpened_<p>.png and sharpen.csv; sharpened[p] is the definition's output for traj[sharpen_source][p] under its mask; with
    sharpen=None every key is the parent's and every shared value is byte for byte the same; without stabilize it is a ValueError"""
    from test_gpu_stabilize_search import TRIALS

    rows, cols, gamma = 16, 64, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    sc = 4.0 / np.abs(f0).max()
    frames, _, _ = rsdsfm.synth.render_sequence(3, rows, cols, K, v * sc, w * sc, k, gamma, seed=21, speeds=(1.0, 1.3))
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=[3, 8], stabilize=True, smooth_sigma=1.0)
    n = len(frames) - 1
    new_keys = {"sharpened", "sharpen_counts", "sharpen_curves", "sharpen_source"}
    with rsdsfm.Solver(0) as s:
        plain = ev(s, frames, out_dir=str(tmp_path / "plain"), **kw)
        sharp = ev(s, frames, sharpen=True, out_dir=str(tmp_path / "sharp"), **kw)
        tuned = ev(s, frames, sharpen=(64, 0, 255), denoise=1, **kw)
        assert set(ev(s, frames, sharpen=None, **kw)) == set(plain) and new_keys.isdisjoint(plain)
        assert set(sharp) == set(plain) | new_keys
        for key in plain:
            if key not in ("pairs", "path_smoothed", "links"):
                assert np.asarray(sharp[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
        assert sharp["sharpen_source"] == "stabilized" and tuned["sharpen_source"] == "stab_denoised"
        assert sharp["sharpen_counts"].shape == (n, 4) and sharp["sharpen_curves"].shape == (n, 9, 4) and len(sharp["sharpened"]) == n
        for res, masks, params in ((sharp, sharp["stab_masks"], (16, 8, 0)), (tuned, tuned["denoise_masks"], (64, 0, 255))):
            for p in range(n):
                want = spec.sharpen_frame(res[res["sharpen_source"]][p], masks[p], *params)
                assert np.array_equal(res["sharpened"][p], want["image"]) and res["sharpen_counts"][p].tolist() == want["counts"], p
                assert res["sharpen_curves"][p].tolist() == want["curve"].astype(np.int64).tolist()
        with pytest.raises(ValueError):
            ev(s, frames, sharpen=True, camera=K, gamma=gamma, trials=TRIALS, seeds=[3, 8])
    lines = open(str(tmp_path / "sharp" / "sharpen.csv")).read().split()
    assert lines[0] == "pair,unset,kept,sharpened,limited,noise_m,strength_min,strength_max" and len(lines) == 1 + n
    lut = nc.noise_curve_strengths(sharp["sharpen_curves"][0].astype(np.uint64))
    assert lines[1].split(",") == ["0"] + [str(int(x)) for x in sharp["sharpen_counts"][0]] + [str(int(sharp["sharpen_curves"][0][8, 1])), str(int(lut.min())), str(int(lut.max()))]
    assert set(os.listdir(str(tmp_path / "sharp"))) == set(os.listdir(str(tmp_path / "plain"))) | {"sharpen.csv"} | {"sharpened_%d.png" % p for p in range(n)}
