"""GPU: the text of the refusals of the estimated-strength denoise -- the noise level ("auto"), the noise curve ("curve") and the temporal
noise curve ("temporal"): their three frame calls, their three clip calls, the four consumers that take a record or a curve and the two
primitives that write one.  The family's own tests accept any RsdsfmError or match a prefix; here one call is made per check, and the message
behind the binding's "... failed (-N): " is compared with the tables below, character for character, as tests/test_gpu_refusal_text.py does for
the stages in front of this family (its helpers are imported).  Calls with two faults at once hold the ORDER of the checks in place: the text
is the one of the fault that is looked at first.

Every expected string occurs verbatim in the source at the commit that added the temporal noise curve ("Temporal noise curve: denoise strength
from registered neighbours"): the stage prefixes and the family's own messages in csrc/noise_host.hip, csrc/noise_curve_host.hip and
csrc/noise_temporal_host.hip, the parameter messages in csrc/denoise_host.hip and csrc/denoise_spatial_host.hip, the top-up's plane
messages in csrc/denoise_spatial_host.hip, and what the shared front, the accumulate check and the clip's array check say in
csrc/clip_stage_host.hip.

The frame and the clip calls run on the smallest case (tests/test_gpu_refusal_text.py's _smallest) of the frame cases that each stage's own
test runs -- tests/noise_cases.py, tests/noise_curve_cases.py and tests/noise_temporal_cases.py hold the primitives' inputs, the frame cases
of all three come from tests/denoise_cases.py -- the consumers and the primitives on 16 x 64 planes (one tile of their kernels).  A refused
call enqueues nothing: the outputs keep their guard bytes.  After each group the faultless call is made once and compared with the definition
as the stage's own test compares it: a refusal leaves no state behind."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_cases as dcases
import denoise_spatial_cases as scases
import noise_cases
import noise_curve_cases
import noise_curve_spec_numpy as cspec
import noise_spec_numpy as nspec
import test_gpu_noise as t_auto
import test_gpu_noise_curve as t_curve
import test_gpu_noise_temporal as t_temporal
from guarded_planes import Plane, fresh
from test_gpu_refusal_text import _front, _null_argument, _refused, _smallest

pytestmark = pytest.mark.gpu

DENOISE_PARAMS = ("rsdsfm_denoise_params: radius in [1, 7] or 0, strength in [1, 255] or 0, gain_mode 0 or 1, occlusion 0 or 1, occlusion_tol_q16 in [0, 65536], "
                  "min_overlap >= 0, struct_bytes 0 or sizeof (use rsdsfm_denoise_params_init)")
SPATIAL_PARAMS = ("rsdsfm_denoise_spatial_params: strength in [1, 255] or 0, target in [1, 255] or 0, search in [1, 3] or 0, struct_bytes 0 or sizeof (use "
                  "rsdsfm_denoise_spatial_params_init)")
NOISE_PARAMS = ("rsdsfm_noise_params: quantile_q8 in [1, 256] or 0, scale in [1, 255] or 0, min_samples >= 0, struct_bytes 0 or sizeof (use "
                "rsdsfm_noise_params_init)")
CURVE_PARAMS = ("rsdsfm_noise_curve_params: quantile_q8 in [1, 256] or 0, scale in [1, 255] or 0, min_samples >= 0, band_min_samples >= 0, struct_bytes 0 or sizeof "
                "(use rsdsfm_noise_curve_params_init)")
NOISE_WORDS = "scale must be in [1, 255] (0: the default, 12) and min_samples >= 0 (0: 1024)"
CURVE_WORDS = "scale must be in [1, 255] (0: the default, 12), min_samples >= 0 (0: 1024) and band_min_samples >= 0 (0: 256)"


def _frame_text(frame, video, noun, params):
    """what a frame call and its clip call say: the nine messages of the shared front (the planes' under the frame's prefix too), then the family's own"""
    return dict(_front(frame, frame), nsrc=frame + ": nsrc must be in [1, 15]", denoise_params=DENOISE_PARAMS, estimator_params=params, spatial_params=SPATIAL_PARAMS,
                support_alone=frame + ": a support plane needs the top-up's parameters", estimate_plus_4=frame + ": the " + noun + " must be 8-byte aligned",
                estimate_is_output=frame + ": an output may not be the " + noun, estimate_is_source=frame + ": null, misaligned or aliased source pointer",
                support_is_image=frame + ": the output planes must be distinct",  # the front refuses it before the top-up's own check is reached
                support_in_counters=frame + ": the outputs must be distinct",    # the top-up's own check, in front of anything enqueued
                clip_null_array=video + ": null array", clip_supports_alone=video + ": the support planes need the top-up's parameters")


TEXT = {
    "auto": _frame_text("denoise auto frame", "denoise auto video", "noise record", NOISE_PARAMS),
    "curve": _frame_text("denoise curve frame", "denoise curve video", "noise curve", CURVE_PARAMS),
    "temporal": _frame_text("denoise temporal frame", "denoise temporal video", "noise curve", CURVE_PARAMS),
}

# the consumers: a null record or curve, one at +4 bytes, one that is an output, scale 256
CONSUMER_TEXT = {
    "auto": dict(accumulate=dict(null="denoise auto accumulate: the noise record is NULL", plus_4="denoise auto accumulate: the cells and the records must be 8-byte aligned",
                                 is_output="denoise auto accumulate: an output may not be an input, a record or the cells", scale="denoise auto accumulate: " + NOISE_WORDS),
                 spatial=dict(null="denoise spatial auto: the noise record is NULL", plus_4="denoise spatial auto: the noise record must be 8-byte aligned",
                              is_output="denoise spatial auto: an output may not be the noise record", scale="denoise spatial auto: " + NOISE_WORDS)),
    "curve": dict(accumulate=dict(null="denoise curve accumulate: the noise curve is NULL", plus_4="denoise curve accumulate: the cells and the records must be 8-byte aligned",
                                  is_output="denoise curve accumulate: an output may not be an input, a record or the cells", scale="denoise curve accumulate: " + CURVE_WORDS),
                  spatial=dict(null="denoise curve spatial: the noise curve is NULL", plus_4="denoise curve spatial: the noise curve must be 8-byte aligned",
                               is_output="denoise curve spatial: an output may not be the noise curve", scale="denoise curve spatial: " + CURVE_WORDS)),
}

PRIMITIVE_TEXT = {
    "auto": dict(null_hist="noise level: null device pointer", hist_is_image="noise level: an output may not be an input", hist_is_estimate="noise level: the outputs must be distinct",
                 estimate_plus_4="noise level: the record must be 8-byte aligned"),
    "curve": dict(null_hist="noise curve: null device pointer", hist_is_image="noise curve: an output may not be an input", hist_is_estimate="noise curve: the outputs must be distinct",
                  estimate_plus_4="noise curve: the curve must be 8-byte aligned"),
}

FAMILIES = ["auto", "curve", "temporal"]


@contextlib.contextmanager
def _argument(lib, name, index, value):
    """test_gpu_refusal_text's _null_argument with any value: the clip wrappers build the parameter structs themselves, a wrong one goes in here"""
    real = getattr(lib, name)

    def shim(*args):
        args = list(args)
        args[index] = value
        return real(*args)

    setattr(lib, name, shim)
    try:
        yield
    finally:
        setattr(lib, name, real)


class Family:
    """one of the three stages: its modules, its binding calls with the solver bound, the keyword of its estimator struct, a wrong struct of each kind"""

    def __init__(self, name, rsdsfm, s):
        import rsdsfm_noise_curve as nc
        import rsdsfm_noise_temporal as nt

        self.name, self.s, self.nc, self.nt = name, s, nc, nt
        self.module = dict(auto=t_auto, curve=t_curve, temporal=t_temporal)[name]
        self.frame = dict(auto=s.denoise_auto_frame_dev, curve=functools.partial(nc.denoise_curve_frame_dev, s), temporal=functools.partial(nt.denoise_temporal_frame_dev, s))[name]
        self.video = dict(auto=s.denoise_auto_video_dev, curve=functools.partial(nc.denoise_curve_video_dev, s), temporal=functools.partial(nt.denoise_temporal_video_dev, s))[name]
        self.words = 4 if name == "auto" else 36
        self.estimator_kw = "noise_params" if name == "auto" else "curve_params"
        self.wrong = dict(denoise=rsdsfm.DenoiseParams(), spatial=rsdsfm.DenoiseSpatialParams(), estimator=rsdsfm.NoiseParams() if name == "auto" else nc.NoiseCurveParams())
        for p in self.wrong.values():  # every word 0, its default; struct_bytes neither 0 nor sizeof
            p.struct_bytes = 4

    def case(self, oracle):
        """the smallest of the frame cases the stage's own test runs"""
        if self.name == "auto":
            return _smallest(dcases.all_cases(oracle.pose_table))
        if self.name == "curve":
            return _smallest([dcases.shift_clip(0, 3), dcases.shift_clip(1, 1)])
        return _smallest([c for c, _ in t_temporal._frame_cases()])

    def check_frame(self, torch, rsdsfm, case):
        """the faultless frame call, as the stage's own test makes and compares it"""
        s, m = self.s, self.module
        if self.name == "auto":
            m._same_frame(m._frame(torch, s, case, top_up=True), m._public_calls(torch, s, rsdsfm, case, top_up=True), "auto")
        elif self.name == "curve":
            m._same_frame(m._frame(torch, s, self.nc, case, top_up=True), m._public_calls(torch, s, self.nc, case, top_up=True), "curve")
        else:
            t_curve._same_frame(m._frame(torch, s, self.nt, case, top_up=True), m._spec_frame(case, top_up=True), "temporal")

    def check_clip(self, torch, case):
        """the faultless clip call: every frame of it is the frame call's, as the stage's own test compares them"""
        s, m = self.s, self.module
        x = dict(auto=(), curve=(self.nc,), temporal=(self.nt,))[self.name]
        got, d, _ = m._video(torch, s, *x, case, True)
        for q in range(len(case["depths"])):
            (t_auto if self.name == "auto" else t_curve)._same_frame(got[q], m._frame(torch, s, *x, case, d, q, True), (self.name, q))


def _outputs(dev, case, words):
    """the four planes 4-byte aligned and not 8 -- the image 8 and not 16, so that it can stand in for the record -- the counters and the estimate 8 and not 16"""
    rows, cols = case["depths"][0].shape
    plane = lambda: fresh((rows, cols), np.uint8, 4, device=dev)
    return dict(image=fresh(case["frames"][0].shape, np.uint8, 8, device=dev), mask=plane(), weight=plane(), support=plane(), counts=fresh((6,), np.int64, 8, device=dev),
                estimate=fresh((words,), np.uint64, 8, device=dev))


class FrameCall:
    """a stage's frame call on its smallest case with the top-up: sources on the device, guarded outputs, and the call with any argument replaced"""

    def __init__(self, torch, fam, case):
        dev = torch.device("cuda", 0)
        self.fam, self.case = fam, case
        self.rows, self.cols = case["depths"][0].shape
        self.ch = 1 if case["frames"][0].ndim == 2 else 3
        self.d = t_curve._clip(torch, dev, case)
        self.src, self.M, self.m = dcases.sources_and_poses(case)
        self.o = _outputs(dev, case, fam.words)
        torch.cuda.synchronize()

    def pick(self, k):
        return [self.d[k][n].data_ptr() for n in self.src]

    def __call__(self, images=None, maps=None, Rs=None, ts=None, M=None, m=None, i=None, k=None, w=None, sp=None, cnt=None, est=None, spatial=True, **kw):
        o, first = self.o, lambda a, b: b if a is None else a
        return self.fam.frame(first(images, self.pick("frames")), self.ch, first(maps, self.pick("maps")), first(Rs, self.pick("Rs")), first(ts, self.pick("ts")), self.case["K"],
                              self.rows, self.cols, first(M, self.M), first(m, self.m), first(i, o["image"].ptr), first(k, o["mask"].ptr), first(w, o["weight"].ptr),
                              first(sp, o["support"].ptr), first(cnt, o["counts"].ptr), first(est, o["estimate"].ptr), spatial=spatial, **kw)

    def sixteen(self):
        """sixteen sources: the case's, repeated"""
        rep = lambda xs: [xs[j % len(xs)] for j in range(16)]
        n = len(self.src)
        return dict(images=rep(self.pick("frames")), maps=rep(self.pick("maps")), Rs=rep(self.pick("Rs")), ts=rep(self.pick("ts")), M=np.array([self.M[j % n] for j in range(16)]),
                    m=np.array([self.m[j % n] for j in range(16)]))

    def untouched(self):
        return all(p.unchanged() for p in self.o.values())


@pytest.mark.parametrize("name", FAMILIES)
def test_a_frame_call_says_what_it_refuses(oracle, rsdsfm, name):
    import torch

    text = TEXT[name]
    with rsdsfm.Solver(0) as s:
        fam = Family(name, rsdsfm, s)
        case = fam.case(oracle)
        call = FrameCall(torch, fam, case)
        o, images = call.o, call.pick("frames")
        nan_M = call.M.copy()
        nan_M.reshape(-1)[0] = np.nan
        lib_name = "rsdsfm_denoise_%s_frame_dev" % name
        with _null_argument(s.lib, lib_name, 1):
            _refused(rsdsfm, call, text["null_array"], "null_array")
        wrong = fam.wrong
        faults = (
            # the nine of the shared front
            ("null_source", dict(images=[0] + images[1:])), ("aliased_source", dict(images=[o["image"].ptr] + images[1:])), ("nan_pose", dict(M=nan_M)),
            ("tall_window", dict(window=(0, 0, call.rows + 1, call.cols))), ("null_image", dict(i=0)), ("mask_is_image", dict(k=o["image"].ptr)),
            ("plane_plus_1", dict(i=o["image"].ptr + 1)), ("counters_plus_4", dict(cnt=o["counts"].ptr + 4)),
            # the family's own
            ("nsrc", dict(images=[])), ("nsrc", call.sixteen()), ("denoise_params", dict(params=wrong["denoise"])), ("estimator_params", {fam.estimator_kw: wrong["estimator"]}),
            ("spatial_params", dict(spatial_params=wrong["spatial"])), ("support_alone", dict(spatial=False)), ("estimate_plus_4", dict(est=o["estimate"].ptr + 4)),
            ("estimate_is_output", dict(est=o["image"].ptr)), ("estimate_is_output", dict(est=o["counts"].ptr)), ("estimate_is_source", dict(est=images[0])),
            ("support_is_image", dict(sp=o["image"].ptr)), ("support_in_counters", dict(sp=o["counts"].ptr + 24)),
            # two faults at once: the one that is looked at first
            ("nsrc", dict(images=[], params=wrong["denoise"])),
            ("estimator_params", {fam.estimator_kw: wrong["estimator"], "images": [0] + images[1:]}),
            ("estimate_plus_4", dict(window=(0, 0, call.rows + 1, call.cols), est=o["estimate"].ptr + 4)),
            ("denoise_params", {"params": wrong["denoise"], fam.estimator_kw: wrong["estimator"]}),
            ("spatial_params", dict(spatial_params=wrong["spatial"], images=[0] + images[1:])),
        )
        for what, bad in faults:
            _refused(rsdsfm, lambda: call(**bad), text[what], (what, sorted(bad)))
        s.synchronize()
        assert call.untouched()  # nothing was enqueued
        fam.check_frame(torch, rsdsfm, case)


@pytest.mark.parametrize("name", FAMILIES)
def test_a_clip_call_says_what_it_refuses(oracle, rsdsfm, name):
    import torch

    text = TEXT[name]
    dev = torch.device("cuda", 0)
    with rsdsfm.Solver(0) as s:
        fam = Family(name, rsdsfm, s)
        case = fam.case(oracle)
        rows, cols = case["depths"][0].shape
        ch = 1 if case["frames"][0].ndim == 2 else 3
        ns = len(case["depths"])
        d = t_curve._clip(torch, dev, case)
        outs = [_outputs(dev, case, fam.words) for _ in range(ns)]
        ptrs = lambda a: [x.data_ptr() for x in a]
        col = lambda k: [o[k].ptr for o in outs]

        def call(sp=None, **kw):
            return fam.video(ptrs(d["frames"]), rows, cols, ch, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"], case["c_path"],
                             case["scales"], col("image"), col("mask"), col("weight"), sp, radius=case["radius"], **kw)

        lib_name = "rsdsfm_denoise_%s_video_dev" % name
        with _null_argument(s.lib, lib_name, 1):
            _refused(rsdsfm, call, text["clip_null_array"], "clip_null_array")
        _refused(rsdsfm, lambda: call(sp=col("support")), text["clip_supports_alone"], "clip_supports_alone")
        # the structs are arguments 21, 22 and 23 of the library's function, the context being 0: params_or_null, noise_or_null / curve_or_null and
        # spatial_or_null of rsdsfm_denoise_{auto,curve,temporal}_video_dev (include/rsdsfm_noise.h, rsdsfm_noise_curve.h, rsdsfm_noise_temporal.h)
        for what, index, struct in (("denoise_params", 21, "denoise"), ("estimator_params", 22, "estimator"), ("spatial_params", 23, "spatial")):
            with _argument(s.lib, lib_name, index, C.byref(fam.wrong[struct])):
                _refused(rsdsfm, call, text[what], what)
        s.synchronize()
        assert all(p.unchanged() for o in outs for p in o.values())  # nothing was enqueued
        fam.check_clip(torch, case)


def _consumer_planes(torch, estimate):
    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    image, mask, weight = scases.frame(rows, cols, 3, seed=2)
    ref, rmask = noise_curve_cases.ramp_reference(rows, cols, 3)
    layers = dcases.layers(ref, rows, cols, 3, 1)
    P = lambda a, al=4: Plane(a, al, device=dev)
    (limg, lmask), = layers
    p = dict(image=P(image), mask=P(mask), weight=P(weight), estimate=P(estimate, 8), ref=P(ref), rmask=P(rmask), layer=P(limg), lmask=P(lmask))
    plane = lambda: fresh((rows, cols), np.uint8, 4, device=dev)
    # the image output 8-byte aligned and not 16, so that it can stand in for the record
    o = dict(image=fresh(image.shape, np.uint8, 8, device=dev), mask=plane(), plane=plane(), counts=fresh((3,), np.int64, 8, device=dev))
    return rows, cols, dict(image=image, mask=mask, weight=weight, ref=ref, rmask=rmask, layers=layers), p, o


@pytest.mark.parametrize("name", ["auto", "curve"])
def test_the_consumers_say_what_they_refuse(rsdsfm, name):
    """the accumulate and the top-up that take a record (auto) or a curve: after the refusals the top-up is the definition's, and the accumulate
    is, as tests/test_gpu_noise.py and tests/test_gpu_noise_curve.py compare them"""
    import torch

    import rsdsfm_noise_curve as nc

    text = CONSUMER_TEXT[name]
    estimate = t_auto._record(5000, 16) if name == "auto" else noise_curve_cases.RISING
    rows, cols, host, p, o = _consumer_planes(torch, estimate)
    with rsdsfm.Solver(0) as s:
        def top_up(n=p["estimate"].ptr, scale=0):
            lead = (p["image"].ptr, p["mask"].ptr, p["weight"].ptr, 3, rows, cols, n, o["image"].ptr, o["plane"].ptr, o["counts"].ptr, 0, scale, 0)
            if name == "auto":
                return s.denoise_spatial_auto_dev(*lead, 0, 0)
            return nc.denoise_spatial_curve_dev(s, *lead, 0, 0, 0)

        def accumulate(n=p["estimate"].ptr, scale=0):
            lead = (p["ref"].ptr, p["rmask"].ptr, p["layer"].ptr, p["lmask"].ptr, 3, rows, cols, None, True, True, n, None, 0, 0, 0, scale, 0)
            tail = (o["image"].ptr, o["mask"].ptr, o["plane"].ptr, o["counts"].ptr)
            if name == "auto":
                return s.denoise_accumulate_auto_dev(*lead, *tail)
            return nc.denoise_accumulate_curve_dev(s, *lead, 0, *tail)

        for fn, which in ((accumulate, "accumulate"), (top_up, "spatial")):
            for what, bad in (("null", dict(n=0)), ("plus_4", dict(n=p["estimate"].ptr + 4)), ("is_output", dict(n=o["image"].ptr)), ("is_output", dict(n=o["counts"].ptr)),
                              ("scale", dict(scale=256)), ("scale", dict(scale=256, n=0))):  # the last: the words are looked at before the record
                _refused(rsdsfm, lambda: fn(**bad), text[which][what], (which, what, sorted(bad)))
        s.synchronize()
        assert all(x.unchanged() for x in o.values())  # nothing was enqueued
        top_up()
        s.synchronize()
        if name == "auto":  # the record asks for 12, the default
            want = s.denoise_spatial(host["image"], host["mask"], host["weight"])
            want = dict(image=want[0], support=want[1], counts=want[2].tolist())
        else:
            want = cspec.denoise_spatial(host["image"], host["mask"], cspec.strengths(estimate), host["weight"])
        assert np.array_equal(o["image"].get(), want["image"]) and np.array_equal(o["plane"].get(), want["support"]) and o["counts"].get().tolist() == want["counts"]
        assert all(x.unchanged() for x in p.values())
        if name == "auto":
            got = t_auto._accumulate_chain(torch, s, host["ref"], host["rmask"], host["layers"], [None], estimate)
            want = t_auto._accumulate_chain(torch, s, host["ref"], host["rmask"], host["layers"], [None], None, nspec.noise_strength(5000, 16, 0, 12, 0))
        else:
            got = t_curve._accumulate_chain(torch, s, nc, host["ref"], host["rmask"], host["layers"], [None], estimate)
            want = cspec.denoise(host["ref"], host["rmask"], host["layers"], cspec.strengths(estimate), [None])
        for key in ("image", "mask", "weight"):
            assert np.array_equal(got[key], want[key]), key
        assert got["counts"] == want["counts"]


@pytest.mark.parametrize("name", ["auto", "curve"])
def test_the_primitives_say_what_they_refuse(rsdsfm, name):
    import torch

    import rsdsfm_noise_curve as nc

    text = PRIMITIVE_TEXT[name]
    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    if name == "auto":
        image, mask = noise_cases.frame(rows, cols, 3, "holes", seed=2)
        hist_shape, words = (nspec.BINS,), (4,)
    else:
        image, mask = noise_curve_cases.frame(rows, cols, 3, "ramp", seed=2)
        hist_shape, words = t_curve.HIST, (9, 4)
    p_i, p_m = Plane(image, 4, device=dev), Plane(mask, 4, device=dev)
    o_h, o_e = fresh(hist_shape, np.uint32, 4, device=dev), fresh(words, np.uint64, 8, device=dev)
    with rsdsfm.Solver(0) as s:
        def call(h=o_h.ptr, e=o_e.ptr):
            if name == "auto":
                return s.noise_level_dev(p_i.ptr, p_m.ptr, 3, rows, cols, h, e, 0)
            return nc.noise_curve_dev(s, p_i.ptr, p_m.ptr, 3, rows, cols, h, e, 0)

        for what, bad in (("null_hist", dict(h=0)), ("hist_is_image", dict(h=p_i.ptr)), ("hist_is_estimate", dict(h=o_e.ptr)), ("estimate_plus_4", dict(e=o_e.ptr + 4)),
                          ("estimate_plus_4", dict(e=o_e.ptr + 4, h=p_i.ptr))):  # the last: the alignment is looked at before the aliases
            _refused(rsdsfm, lambda: call(**bad), text[what], (what, sorted(bad)))
        s.synchronize()
        assert o_h.unchanged() and o_e.unchanged()  # nothing was enqueued
        call()
        s.synchronize()
        if name == "auto":
            want = nspec.noise_level(image, mask)
            assert np.array_equal(o_h.get(), want["hist"]) and o_e.get().tolist() == want["record"].tolist()
        else:
            want = cspec.noise_curve(image, mask)
            assert np.array_equal(o_h.get(), want["hist"]) and o_e.get().tolist() == want["curve"].tolist()
        assert p_i.unchanged() and p_m.unchanged()
