"""GPU: the temporal noise curve (include/rsdsfm_noise_temporal.h) bit for bit against its definition (tests/noise_temporal_spec_numpy.py) in
both library builds -- the pair histogram at the shapes where its 16 x 64 tile, its byte paths and its halo can go wrong, with holes, saturated
bytes, gains other than 1, an empty layer, two layers in both orders and a preset histogram; the resolve alone against rsdsfm_noise_curve_dev's
own curve; the frame call against the public calls made one after another and against the definition; the clip call against the frame calls;
and the refusals.  Every plane sits at the minimum alignment the header admits between guard bytes (tests/guarded_planes.py); the outputs are
never preset and the inputs are verified unchanged.  The helpers of tests/test_gpu_noise_curve.py are imported as they are."""
import numpy as np
import pytest

import denoise_cases as dcases
import noise_curve_cases as ccases
import noise_curve_spec_numpy as cspec
import noise_temporal_cases as cases
import noise_temporal_spec_numpy as spec
import shutter_cases as scases
import test_gpu_noise_curve as base
from guarded_planes import Plane, fresh

pytestmark = pytest.mark.gpu

HIST = (spec.BANDS, spec.BINS)
SPATIAL = base.SPATIAL
SPATIAL_SPEC = dict(strength=SPATIAL["spatial_strength"], target=SPATIAL["target"], search=SPATIAL["search"])
# the cases are small: the defaults (1024 and 256 samples) are more than some of them have
CURVE_KW = dict(min_samples=ccases.MIN_SAMPLES, band_min_samples=ccases.BAND_MIN_SAMPLES)


@pytest.fixture(scope="module")
def nt():
    import rsdsfm_noise_temporal

    return rsdsfm_noise_temporal


@pytest.fixture(scope="module")
def nc():
    import rsdsfm_noise_curve

    return rsdsfm_noise_curve


def _dev(torch):
    return torch.device("cuda", 0)


def _ch(image):
    return 1 if image.ndim == 2 else 3


# ---------------------------------------------------------------------------------------------------
# the pair histogram and the resolve
# ---------------------------------------------------------------------------------------------------
def _pair_hist(torch, s, nt, ref, rmask, layers, records=None, min_overlap=0, gain_mode=0, o_h=None):
    """the layers one after another into one histogram (first on the first) -> (8, 1024) uint32"""
    dev = _dev(torch)
    rows, cols = rmask.shape
    p_r, p_m = Plane(ref, 4, device=dev), Plane(rmask, 4, device=dev)
    p_l = [(Plane(i, 4, device=dev), Plane(m, 4, device=dev)) for i, m in layers]
    p_rec = [Plane(r, 8, device=dev) if records is not None and r is not None else None for r in (records if records is not None else [None] * len(layers))]
    o_h = o_h or fresh(HIST, np.uint32, 4, device=dev)
    for j, (li, lm) in enumerate(p_l):
        nt.noise_pair_hist_dev(s, p_r.ptr, p_m.ptr, li.ptr, lm.ptr, _ch(ref), rows, cols, o_h.ptr, j == 0, p_rec[j].ptr if p_rec[j] else None, min_overlap, gain_mode)
    s.synchronize()
    assert p_r.unchanged() and p_m.unchanged() and all(a.unchanged() and b.unchanged() for a, b in p_l) and all(r is None or r.unchanged() for r in p_rec)
    return o_h.get()


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_pair_histogram_equals_the_definition(rsdsfm, nt, arith):
    """every shape of noise_temporal_cases.PAIR_SHAPES x one and three channels x full masks, holes, saturated bytes in R and in L and an empty
    layer mask, into a histogram that was never preset; a record that gives gains other than 1, then gain_mode = 1, then no record; two layers
    in both orders; first = 1 on a histogram preset to 0xFF"""
    import torch

    with rsdsfm.Solver(0, arith=arith) as s:
        every = cases.pair_cases()
        assert {c["ref"].shape[:2] for c in every} == set(cases.PAIR_SHAPES) and {c["kind"] for c in every} == set(cases.PAIR_KINDS)
        samples = {}
        for case in every:
            want = cases.run_spec(case)
            got = _pair_hist(torch, s, nt, case["ref"], case["rmask"], [(case["layer"], case["lmask"])])
            assert np.array_equal(got, want), case["name"]
            samples[case["name"]] = int(want.sum())
        assert samples["2x2x3-full"] == 0 and samples["3x3x1-full"] == 1 and samples["16x64x3-full"] == 14 * 62 and samples["17x65x1-full"] == 15 * 63
        assert 0 < samples["33x130x3-holes"] < 31 * 128 and 0 < samples["33x130x1-saturated"] < 31 * 128 and samples["33x130x3-empty"] == 0

        g = dcases.run_spec(dcases.gained_clip())  # 37 x 67, neighbours brighter and darker than the own frame
        ref, rmask, _ = g["ref"]
        recs = list(g["records"])
        assert all(G != [65536] * 3 for G in (spec.temporal.gains(r, 3) for r in recs))
        hists = []
        for kw in (dict(records=recs), dict(records=recs, gain_mode=1), dict(records=None), dict(records=recs, min_overlap=100000)):
            got = _pair_hist(torch, s, nt, ref, rmask, g["layers"], **kw)
            assert np.array_equal(got, spec.frame_histogram(ref, rmask, g["layers"], kw["records"], kw.get("min_overlap", 0) or spec.MIN_OVERLAP_DEFAULT, kw.get("gain_mode", 0))), kw
            hists.append(got)
        assert hists[0].sum() > 0 and not np.array_equal(hists[0], hists[1]) and np.array_equal(hists[1], hists[2]) and np.array_equal(hists[2], hists[3])

        ref, rmask, _, _ = cases.pair(33, 130, 3, "holes", seed=5)
        layers = [cases.pair(33, 130, 3, "holes", seed=5, amp=a)[2:] for a in (2, 11)]
        want = spec.frame_histogram(ref, rmask, layers)
        for order in (layers, layers[::-1]):
            assert np.array_equal(_pair_hist(torch, s, nt, ref, rmask, order), want)
        preset = Plane(np.full(HIST, 0xFFFFFFFF, dtype=np.uint32), 4, device=_dev(torch))
        assert np.array_equal(_pair_hist(torch, s, nt, ref, rmask, layers, o_h=preset), want)
        assert nt.noise_pair_hist_launches() == 1 and nt.noise_curve_resolve_launches() == 1
        r = nt.noise_temporal(s, ref, rmask, layers, min_samples=ccases.MIN_SAMPLES, band_min_samples=ccases.BAND_MIN_SAMPLES)  # the host convenience
        assert np.array_equal(r["hist"], want) and r["curve"].tolist() == spec.resolve(want).tolist()
        assert np.array_equal(r["lut"], cspec.strengths(r["curve"], 0, 12, ccases.MIN_SAMPLES, ccases.BAND_MIN_SAMPLES))


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_resolve_equals_the_noise_curves_own(rsdsfm, nt, nc, arith):
    """on the histogram rsdsfm_noise_curve_dev wrote, the resolve alone gives that call's curve, at three quantiles; on a pair histogram it gives
    the definition's"""
    import torch

    dev = _dev(torch)
    with rsdsfm.Solver(0, arith=arith) as s:
        for k, q in enumerate((0, 64, 256)):
            image, mask = ccases.frame(18, 66, 3 if k % 2 == 0 else 1, "ramp", seed=k)
            p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
            o_h, o_c, o_c2 = fresh(HIST, np.uint32, 4, device=dev), fresh((9, 4), np.uint64, 8, device=dev), fresh((9, 4), np.uint64, 8, device=dev)
            nc.noise_curve_dev(s, p_i.ptr, p_m.ptr, _ch(image), 18, 66, o_h.ptr, o_c.ptr, q)
            s.synchronize()
            hist = o_h.get()
            nt.noise_curve_resolve_dev(s, o_h.ptr, o_c2.ptr, q)
            s.synchronize()
            assert hist.sum() > 0 and o_c2.get().tolist() == o_c.get().tolist() == cspec.resolve(hist, q).tolist() and np.array_equal(o_h.get(), hist)


def test_primitive_argument_errors(rsdsfm, nt):
    """every refusal is RSDSFM_ERR_INVALID with its prefix and enqueues nothing: the outputs keep their guard bytes; after the refused calls the
    same calls without the fault go through"""
    import torch

    dev = _dev(torch)
    rows, cols = 17, 65
    ref, rmask, layer, lmask = cases.pair(rows, cols, 3, "holes", seed=2)
    P = lambda a, al=4: Plane(a, al, device=dev)
    p_r, p_m, p_l, p_k, p_s = P(ref), P(rmask), P(layer), P(lmask), P(np.zeros(8, dtype=np.uint64), 8)
    o_h, o_c = fresh(HIST, np.uint32, 4, device=dev), fresh((9, 4), np.uint64, 8, device=dev)
    with rsdsfm.Solver(0) as s:
        def call(r=p_r.ptr, m=p_m.ptr, l=p_l.ptr, k=p_k.ptr, ch=3, ro=rows, co=cols, h=o_h.ptr, first=True, rec=p_s.ptr, mo=0, gm=0):
            return nt.noise_pair_hist_dev(s, r, m, l, k, ch, ro, co, h, first, rec, mo, gm)

        bads = (dict(r=0), dict(m=0), dict(l=0), dict(k=0), dict(h=0), dict(r=p_r.ptr + 1), dict(m=p_m.ptr + 2), dict(l=p_l.ptr + 1), dict(k=p_k.ptr + 2), dict(h=o_h.ptr + 2),
                dict(rec=p_s.ptr + 4), dict(h=p_r.ptr), dict(h=p_m.ptr), dict(h=p_l.ptr), dict(h=p_k.ptr), dict(h=p_s.ptr), dict(l=p_r.ptr), dict(k=p_m.ptr), dict(m=p_r.ptr),
                dict(ch=2), dict(ch=4), dict(ro=1), dict(co=1), dict(ro=16385), dict(co=16385), dict(mo=-1), dict(gm=2), dict(first=2))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError, match="noise pair: "):
                call(**bad)
        for bad in (dict(h=0), dict(c=0), dict(h=o_h.ptr + 2), dict(c=o_c.ptr + 4), dict(c=o_h.ptr), dict(q=-1), dict(q=257)):
            kw = dict(dict(h=o_h.ptr, c=o_c.ptr, q=0), **bad)
            with pytest.raises(rsdsfm.RsdsfmError, match="noise resolve: "):
                nt.noise_curve_resolve_dev(s, kw["h"], kw["c"], kw["q"])
        s.synchronize()
        assert o_h.unchanged() and o_c.unchanged()  # nothing was enqueued
        call(rec=None)
        nt.noise_curve_resolve_dev(s, o_h.ptr, o_c.ptr)
        s.synchronize()
        want = spec.noise_temporal(ref, rmask, [(layer, lmask)])
        assert np.array_equal(o_h.get(), want["hist"]) and o_c.get().tolist() == want["curve"].tolist() and want["hist"].sum() > 0
        assert all(p.unchanged() for p in (p_r, p_m, p_l, p_k, p_s))


# ---------------------------------------------------------------------------------------------------
# the frame call and the clip call
# ---------------------------------------------------------------------------------------------------
def _frame(torch, s, nt, case, d=None, q=None, top_up=False, with_optional=True, curve_kw=CURVE_KW):
    """one rsdsfm_denoise_temporal_frame_dev of frame q of a case into guarded, never preset outputs"""
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    d = d or base._clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case, q)
    o = base._outputs(dev, case)
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    opt = lambda k: o[k].ptr if with_optional else None
    nt.denoise_temporal_frame_dev(s, pick("frames"), _ch(case["frames"][0]), pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, o["image"].ptr, o["mask"].ptr,
                                  opt("weight"), opt("support") if top_up else None, opt("counts"), opt("curve"), **base._frame_kw(case), **curve_kw,
                                  **(SPATIAL if top_up else {}))
    s.synchronize()
    for t, a in zip(d["frames"], case["frames"]):
        assert np.array_equal(t.cpu().numpy(), a)
    return base._collect(o, top_up, with_optional)


def _spec_frame(case, q=None, top_up=False, curve_kw=CURVE_KW):
    """the definition on frame q of a case, in _collect's form"""
    src, M, m = dcases.sources_and_poses(case, q)
    pick = lambda k: [case[k][n] for n in src]
    r = spec.denoise_temporal_frame(pick("frames"), pick("depths"), pick("Rs"), pick("ts"), case["K"], M, m, case["window"], case["strength"], case["min_overlap"],
                                    case["gain_mode"], case["occlusion"], case["search"], case["tol_q16"], case["mode"], case["q5_mode"], case["iterations"],
                                    spatial=SPATIAL_SPEC if top_up else None, **curve_kw)
    return dict(image=r["image"], mask=r["mask"], weight=r["weight"], support=r["support"] if top_up else None,
                counts=r["counts"] + (r["spatial_counts"] if top_up else [0, 0, 0]), curve=r["curve"].tolist(), lut=r["lut"], spec=r, nsrc=len(src))


def _public_calls(torch, s, nt, nc, case, want, q=None, top_up=False, curve_kw=CURVE_KW):
    """what the frame call promises to equal, public calls one after another on planes of the test's own: the rendered reference planes (the
    existing frame call on the own frame alone), per neighbour rsdsfm_noise_pair_hist_dev on the layer and the record the definition renders
    (tests/test_gpu_denoise.py holds the library's renders to it byte for byte), one rsdsfm_noise_curve_resolve_dev, then
    rsdsfm_denoise_accumulate_curve_dev per neighbour and rsdsfm_denoise_spatial_curve_dev"""
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    ch = _ch(case["frames"][0])
    d = base._clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case, q)
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    ref, rmask = fresh(case["frames"][0].shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev)
    s.denoise_frame_dev(pick("frames")[:1], ch, pick("maps")[:1], pick("Rs")[:1], pick("ts")[:1], case["K"], rows, cols, M[:1], m[:1], ref.ptr, rmask.ptr, **base._frame_kw(case))
    s.synchronize()
    r = want["spec"]
    assert np.array_equal(ref.get(), r["ref"][0]) and np.array_equal(rmask.get(), r["ref"][1])
    layers, records = r["layers"], list(r["records"])
    if layers:
        hist = _pair_hist(torch, s, nt, ref.get(), rmask.get(), layers, records, case["min_overlap"], case["gain_mode"])
    else:
        hist = np.zeros(HIST, dtype=np.uint32)
    p_h, cur = Plane(hist, 4, device=dev), fresh((9, 4), np.uint64, 8, device=dev)
    nt.noise_curve_resolve_dev(s, p_h.ptr, cur.ptr)
    s.synchronize()
    curve = cur.get()
    kw = dict(strength=case["strength"], scale=curve_kw.get("scale", 0), min_samples=curve_kw.get("min_samples", 0), band_min_samples=curve_kw.get("band_min_samples", 0))
    acc = base._accumulate_chain(torch, s, nc, ref.get(), rmask.get(), layers, records, curve, **kw)
    out = dict(image=acc["image"], mask=acc["mask"], weight=acc["weight"], support=None, counts=acc["counts"] + [0, 0, 0], curve=curve.tolist())
    if top_up:
        P = lambda a, al=4: Plane(a, al, device=dev)
        p_i, p_m, p_w, p_n = P(acc["image"]), P(acc["mask"]), P(acc["weight"]), P(curve, 8)
        o_i, o_s, o_c = fresh(acc["image"].shape, np.uint8, 4, device=dev), fresh((rows, cols), np.uint8, 4, device=dev), fresh((3,), np.int64, 8, device=dev)
        nc.denoise_spatial_curve_dev(s, p_i.ptr, p_m.ptr, p_w.ptr, ch, rows, cols, p_n.ptr, o_i.ptr, o_s.ptr, o_c.ptr, SPATIAL["spatial_strength"], kw["scale"], kw["min_samples"],
                                     kw["band_min_samples"], SPATIAL["target"], SPATIAL["search"])
        s.synchronize()
        out.update(image=o_i.get(), support=o_s.get(), counts=acc["counts"] + o_c.get().tolist())
    return out


def _frame_cases():
    """(case, q): the 24 x 40 shift clip with five sources (BGR, from its middle), two (gray, radius 1 from its first frame) and one (a clip of
    one frame), and a fold clip through the occlusion test"""
    return [(dcases.shift_clip(0, 3), None), (dcases.shift_clip(1, 1, q=0, radius=1), None), (dcases.shift_clip(2, 3, q=0, nframes=1), None),
            (dcases.from_shutter(scases.fold_clip(24, 40, 3, 1, 0), "fold-visible", 1, radius=1, occlusion=1), None)]


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_frame_call_equals_the_public_calls_and_the_definition(rsdsfm, nt, nc, arith):
    """nsrc = 5, 2 and 1 on the shift clip and a fold clip through occlusion = 1, with and without the top-up, with and without the optional
    outputs (the caller's curve buffer among them); the defaults (1024 samples or the fallback) once"""
    import torch

    nsrcs, tables = set(), set()
    with rsdsfm.Solver(0, arith=arith) as s:
        for case, q in _frame_cases():
            rows, cols = case["depths"][0].shape
            for top_up in (False, True):
                want = _spec_frame(case, q, top_up)
                nsrcs.add(want["nsrc"])
                tables.add(len(set(want["lut"].tolist())))
                base._same_frame(_public_calls(torch, s, nt, nc, case, want, q, top_up), want, (case["name"], top_up, "public"))
                base._same_frame(_frame(torch, s, nt, case, q=q, top_up=top_up), want, (case["name"], top_up))
                base._same_frame(_frame(torch, s, nt, case, q=q, top_up=top_up, with_optional=False), want, (case["name"], top_up, "bare"))
                assert nt.denoise_temporal_frame_launches(rows, cols, want["nsrc"], top_up) == rsdsfm.denoise_launches(rows, cols, want["nsrc"]) + want["nsrc"] + int(top_up)
        case = dcases.shift_clip(0, 3)
        want = _spec_frame(case, curve_kw=dict())
        assert int(np.asarray(want["curve"])[8][0]) >= 1024  # the defaults use the curve here
        base._same_frame(_frame(torch, s, nt, case, curve_kw=dict()), want, "defaults")
    assert {1, 2, 5} <= nsrcs and max(tables) > 1


def test_frame_argument_errors(rsdsfm, nt, nc):
    """a refused frame call enqueues nothing: the outputs keep their guard bytes; the valid call behind them gives the definition's bytes"""
    import torch

    dev = _dev(torch)
    case = dcases.shift_clip(0, 3)
    rows, cols = case["depths"][0].shape
    d = base._clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case)
    o = base._outputs(dev, case)
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    with rsdsfm.Solver(0) as s:
        def call(images=pick("frames"), maps=pick("maps"), M=M, m=m, i=o["image"].ptr, k=o["mask"].ptr, w=o["weight"].ptr, sp=o["support"].ptr, cnt=o["counts"].ptr,
                 cv=o["curve"].ptr, ch=3, spatial=True, **kw):
            return nt.denoise_temporal_frame_dev(s, images, ch, maps, pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, i, k, w, sp, cnt, cv, spatial=spatial, **kw)

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
        base._same_frame(base._collect(o, True), _spec_frame(case, top_up=True))


def test_evaluate_real_sequence_with_the_temporal_curve(rsdsfm, nt, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, denoise=(K, "temporal"[, spatial])) behaves as "curve" does: the same keys, the same files and
    the same columns of denoise.csv, with the curve of the registered neighbours in denoise_curve"""
    import os

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
        temporal = ev(s, frames, denoise=(2, "temporal"), out_dir=str(tmp_path / "temporal"), **kw)
        topped = ev(s, frames, denoise=(2, "temporal", True), **kw)
        curved = ev(s, frames, denoise=(2, "curve"), out_dir=str(tmp_path / "curve"), **kw)
    assert set(temporal) == set(curved) and set(topped) == set(curved) | {"denoise_support", "denoise_spatial_counts"}
    curve = temporal["denoise_curve"]
    assert curve.shape == (n, 9, 4) and curve.dtype == np.int64 and np.array_equal(curve, topped["denoise_curve"])
    assert (curve[:, :8, 0].sum(axis=1) == curve[:, 8, 0]).all() and not np.array_equal(curve, curved["denoise_curve"])
    for key in curved:
        if key not in ("pairs", "path_smoothed", "links", "stab_denoised", "denoise_masks", "denoise_weights", "denoise_counts", "denoise_curve"):
            assert np.asarray(temporal[key]).tobytes() == np.asarray(curved[key]).tobytes(), key
    lines = open(str(tmp_path / "temporal" / "denoise.csv")).read().split()
    assert lines[0] == open(str(tmp_path / "curve" / "denoise.csv")).read().split()[0] and len(lines) == 1 + n
    import rsdsfm_noise_curve as nc

    lut = nc.noise_curve_strengths(curve[0].astype(np.uint64))
    assert lines[1].split(",")[5:] == [str(int(x)) for x in curve[0, :, 1]] + [str(int(lut.min())), str(int(lut.max()))]
    assert set(os.listdir(str(tmp_path / "temporal"))) == set(os.listdir(str(tmp_path / "curve")))


def _video(torch, s, nt, case, top_up, want_counts=True, want_curves=True, with_optional=True):
    dev = _dev(torch)
    rows, cols = case["depths"][0].shape
    ns = len(case["depths"])
    d = base._clip(torch, dev, case)
    outs = [base._outputs(dev, case) for _ in range(ns)]
    ptrs = lambda a: [x.data_ptr() for x in a]
    col = lambda k: [o[k].ptr for o in outs]
    r = nt.denoise_temporal_video_dev(s, ptrs(d["frames"]), rows, cols, _ch(case["frames"][0]), case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"],
                                      case["A_path"], case["c_path"], case["scales"], col("image"), col("mask"), col("weight") if with_optional else None,
                                      col("support") if with_optional and top_up else None, want_counts=want_counts, want_curves=want_curves, radius=case["radius"],
                                      **base._frame_kw(case), **CURVE_KW, **(SPATIAL if top_up else {}))
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
def test_the_clip_call_equals_the_frame_calls(rsdsfm, nt, arith):
    """the shift clip's five frames of 24 x 40 at radius 2 (one-sided neighbours at the ends, so the stack grows along the walk), BGR with and
    gray without the top-up: every frame of the clip call is the frame call's, counters and curves included; with neither host array the call
    only enqueues; a refused call enqueues nothing"""
    import torch

    with rsdsfm.Solver(0, arith=arith) as s:
        for case, top_up in ((dcases.shift_clip(0, 3), True), (dcases.shift_clip(1, 1), False)):
            got, d, _ = _video(torch, s, nt, case, top_up)
            for q in range(len(case["depths"])):
                base._same_frame(got[q], _frame(torch, s, nt, case, d, q, top_up), (case["name"], q))
            base._same_frame(got[2], _spec_frame(case, 2, top_up), (case["name"], "definition"))
        case = dcases.shift_clip(0, 3)
        full, _, _ = _video(torch, s, nt, case, True)
        for kw in (dict(want_counts=False), dict(want_counts=False, want_curves=False, with_optional=False)):
            got, _, _ = _video(torch, s, nt, case, True, **kw)
            for q in range(len(case["depths"])):
                base._same_frame(got[q], full[q], (q, kw))
        dev = _dev(torch)
        rows, cols = case["depths"][0].shape
        ns = len(case["depths"])
        d = base._clip(torch, dev, case)
        outs = [base._outputs(dev, case) for _ in range(ns)]
        ptrs = lambda a: [x.data_ptr() for x in a]
        bad_scales = case["scales"].copy()
        bad_scales[ns - 1] = 0.0

        def call(scales=case["scales"], i=None, sp=None, **kw):
            return nt.denoise_temporal_video_dev(s, ptrs(d["frames"]), rows, cols, 3, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"],
                                                 case["c_path"], scales, i or [o["image"].ptr for o in outs], [o["mask"].ptr for o in outs], None, sp, **kw)

        for bad in (dict(scales=bad_scales), dict(radius=8), dict(strength=300), dict(spatial=True, search=4), dict(scale=256), dict(quantile_q8=300), dict(min_samples=-1),
                    dict(band_min_samples=-1), dict(i=[outs[0]["image"].ptr] * (ns - 1) + [0]), dict(sp=[o["support"].ptr for o in outs]),
                    dict(i=[outs[0]["image"].ptr] * (ns - 1) + [d["frames"][1].data_ptr()])):
            with pytest.raises(rsdsfm.RsdsfmError, match="denoise temporal video|rsdsfm_"):
                call(**bad)
        s.synchronize()
        assert all(p.unchanged() for o in outs for p in o.values())
