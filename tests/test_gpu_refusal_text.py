"""GPU: the text of the refusals that the frame calls and the accumulate calls of the temporal image stages share (csrc/clip_stage_host.hpp's
front of a frame call, its output planes check and the accumulate check).  Every other test accepts any RsdsfmError; here one call is made
per shared check and stage -- a null source array, a null source, a source that is the image output, a NaN pose, a window one row too tall, a
null image output, the mask output equal to the image output, an output plane at +1 byte, the counters at +4 bytes -- and the message behind the
binding's "... failed (-N): " is compared with the tables below, character for character.

Every expected string occurs verbatim in the source of its stage at the commit before the checks were shared ("Sharpness transfer: a blurred
frame takes its sharper neighbours' pixels"): `git show <that commit>:rs-aware-differential-sfm_amd/csrc/<stage>_host.hip` and a text search
find each of them -- the "plate frame: ..." strings of the erase's table in plate_host.hip, whose frame call the erase calls, the "retime
merge: ..." strings in retime_host.hip.

The frame calls run on the smallest case of each stage's *_cases.py, the accumulate calls on 16 x 64 planes (one tile of their kernels).  A
refused call enqueues nothing, and after each group the faultless call is made once and compared with the stage's definition as the stage's
own tests compare it: a refusal leaves no state behind.  Counters that are one of the output planes are accepted by the denoise, the deblur
and the super-resolution and refused by the plate and the erase (DESIGN's known gaps): the last test holds that difference in place."""
import contextlib

import numpy as np
import pytest

import deblur_cases
import denoise_cases
import erase_cases
import plate_cases
import retime_cases
import superres_cases
import test_gpu_deblur as t_deblur
import test_gpu_denoise as t_denoise
import test_gpu_erase as t_erase
import test_gpu_plate as t_plate
import test_gpu_plate_medoid as t_medoid
import test_gpu_retime as t_retime
import test_gpu_superres as t_superres

pytestmark = pytest.mark.gpu

GUARD = 0xCD
WINDOW = "the window (r0, c0, h, w) needs h >= 1, w >= 1 and must lie inside the frame"


def _front(frame, planes):
    """the nine messages of a frame call whose own front makes every check: `frame` prefixes the sources', poses' and window's, `planes` the outputs'"""
    return dict(null_array=frame + ": null source array", null_source=frame + ": null, misaligned or aliased source pointer",
                aliased_source=frame + ": null, misaligned or aliased source pointer", nan_pose=frame + ": the poses (M, m) must be given and finite",
                tall_window=frame + ": " + WINDOW, null_image=planes + ": null output plane", mask_is_image=planes + ": the output planes must be distinct",
                plane_plus_1=planes + ": every plane must be 4-byte aligned", counters_plus_4=planes + ": the counters must be 8-byte aligned")


FRAME_TEXT = {
    "denoise": _front("denoise frame", "denoise"),
    "deblur": _front("deblur frame", "deblur"),
    "superres": _front("superres frame", "superres"),
    "plate": _front("plate frame", "plate"),
    "retime": _front("retime frame", "retime merge"),  # the merge's check is the frame call's check of its outputs
    # the erase checks its outputs and its sources against them; the sources themselves, the poses and the window are the plate call's to refuse
    "erase": dict(_front("plate frame", "erase"), null_array="erase frame: null source array", aliased_source="erase frame: a source image may not be an output"),
}

# the four checks of the outputs as an accumulate call (the plate: the estimator call) words them, and what the shared accumulate check adds
ACCUMULATE_TEXT = {
    "denoise": dict(null_image="denoise: null output plane", mask_is_image="denoise: the output planes must be distinct", plane_plus_1="denoise: every plane must be 4-byte aligned",
                    counters_plus_4="denoise: the counters must be 8-byte aligned", first_2="denoise accumulate: first and last must be 0 or 1",
                    null_reference="denoise accumulate: the reference needs its image and its mask", null_layer_mask="denoise accumulate: the layer needs its image and its mask, or neither",
                    layer_is_reference="denoise accumulate: the reference's and the layer's planes must be distinct", null_cells="denoise accumulate: the cells may be NULL only with first and last",
                    reference_plus_1="denoise: every plane must be 4-byte aligned", record_plus_4="denoise accumulate: the cells and the record must be 8-byte aligned",
                    image_is_reference="denoise accumulate: an output may not be an input, the record or the cells", cells_are_reference="denoise accumulate: the cells may not be an input plane"),
    "deblur": dict(null_image="deblur: null output plane", mask_is_image="deblur: the output planes must be distinct", plane_plus_1="deblur: every plane must be 4-byte aligned",
                   counters_plus_4="deblur: the counters must be 8-byte aligned", first_2="deblur accumulate: first and last must be 0 or 1",
                   null_reference="deblur accumulate: the reference needs its image and its mask", null_layer_mask="deblur accumulate: the layer needs its image and its mask, or neither",
                   layer_is_reference="deblur accumulate: the reference's and the layer's planes must be distinct", null_cells="deblur accumulate: the cells may be NULL only with first and last",
                   reference_plus_1="deblur: every plane must be 4-byte aligned", record_plus_4="deblur accumulate: the cells and the records must be 8-byte aligned",
                   image_is_reference="deblur accumulate: an output may not be an input, a record or the cells", cells_are_reference="deblur accumulate: the cells may not be an input plane or a record",
                   null_sharpness="deblur accumulate: a layer needs its sharpness record", cells_are_record="deblur accumulate: the cells may not be an input plane or a record"),
    "superres": dict(null_image="superres: null output plane", mask_is_image="superres: the output planes must be distinct", plane_plus_1="superres: every plane must be 4-byte aligned",
                     counters_plus_4="superres: the counters must be 8-byte aligned"),
    "plate": dict(null_image="plate: null output plane", mask_is_image="plate: the output planes must be distinct", plane_plus_1="plate: every plane must be 4-byte aligned",
                  counters_plus_4="plate: the counters must be 8-byte aligned"),
}

COUNTERS_ARE_A_PLANE = {"denoise": None, "deblur": None, "superres": None, "plate": "plate: the output planes must be distinct", "erase": "erase: the output planes must be distinct"}


def _refused(rsdsfm, call, want, what):
    with pytest.raises(rsdsfm.RsdsfmError) as e:
        call()
    head, _, text = str(e.value).partition("): ")
    assert " failed (-" in head and text == want, (what, str(e.value))


@contextlib.contextmanager
def _null_argument(lib, name, index):
    """the binding builds the source arrays itself and cannot pass a null one: the library's function is reached through a shim that does"""
    real = getattr(lib, name)

    def shim(*args):
        args = list(args)
        args[index] = None
        return real(*args)

    setattr(lib, name, shim)
    try:
        yield
    finally:
        setattr(lib, name, real)


def _smallest(all_cases):
    return min(all_cases, key=lambda c: c["depths"][0].size)


# per stage: its cases, its own test module (for the faultless call and the comparison), the planes behind the mask, the binding's arguments
# behind the counters, the upscaling of its outputs
class Stage:
    def __init__(self, name, cases, module, extras, tail=(), scaled=False):
        self.name, self.cases, self.module, self.extras, self.tail, self.scaled = name, cases, module, extras, tail, scaled

    def case(self, oracle):
        return _smallest(self.cases.all_cases(oracle.pose_table))

    def sources(self, case):
        if self.name == "retime":
            return list(range(len(case["images"]))), np.array(case["M"], dtype=np.float64).reshape(-1, 3, 3), np.array(case["m"], dtype=np.float64).reshape(-1, 3)
        poses = self.cases.sources_and_poses if hasattr(self.cases, "sources_and_poses") else denoise_cases.sources_and_poses
        src, M, m = poses(case)
        return list(src), np.array(M, dtype=np.float64), np.array(m, dtype=np.float64)

    def keywords(self, case):
        if self.name == "retime":
            return dict(window=case["window"], threshold=case["threshold"], occlusion=case["occlusion"], occlusion_tol_q16=case["tol_q16"], mode=case["mode"],
                        q5_mode=case["q5_mode"], iterations=case["iterations"])
        return self.module._frame_kw(case)

    def want(self, case):
        return self.cases.run_spec(case)

    def check(self, torch, s, case):
        """the faultless call, as the stage's own tests make and compare it"""
        got = self.module._frame(torch, s, case)
        want = self.want(case)
        if self.name == "erase":
            self.module._same(got, want, self.name, t_erase.PLANES)
        else:
            self.module._same(got, want, self.name)


class Medoid(Stage):
    def want(self, case):  # the fixture the CPU suite holds to the medoid's definition, as tests/test_gpu_plate_medoid.py compares
        return t_plate._golden(np.load(t_medoid.GOLDEN), case["name"])


STAGES = [Stage("denoise", denoise_cases, t_denoise, 1), Stage("deblur", deblur_cases, t_deblur, 1, tail=(None,)), Stage("superres", superres_cases, t_superres, 1, scaled=True),
          Stage("plate", plate_cases, t_plate, 2), Medoid("plate", plate_cases, t_plate, 2), Stage("erase", erase_cases, t_erase, 2), Stage("retime", retime_cases, t_retime, 1)]
IDS = ["denoise", "deblur", "superres", "plate-median", "plate-medoid", "erase", "retime"]


class FrameCall:
    """one stage's frame call on its smallest case: sources on the device, output planes of GUARD bytes, and the call with any argument replaced"""

    def __init__(self, torch, s, st, case):
        dev = torch.device("cuda", 0)
        self.s, self.st, self.case = s, st, case
        self.rows, self.cols = case["depths"][0].shape
        host = case["images" if st.name == "retime" else "frames"]
        self.ch = 1 if host[0].ndim == 2 else 3
        src, self.M, self.m = st.sources(case)
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.keep = [[tt(host[n]) for n in src], [tt(case["depths"][n].T) for n in src], [tt(np.asarray(case["Rs"][n]).reshape(-1, 9)) for n in src], [tt(case["ts"][n]) for n in src]]
        self.images, self.maps, self.Rs, self.ts = ([x.data_ptr() for x in xs] for xs in self.keep)
        S = case["scale"] if st.scaled else 1
        shape = (S * self.rows, S * self.cols)
        # 64 bytes at least behind every plane: the counters that test_counters_that_are_an_output_plane lays over one fit the smallest case's too
        u8 = lambda *sh: torch.full((max(int(np.prod(sh)), 64),), GUARD, dtype=torch.uint8, device=dev)[:int(np.prod(sh))].view(*sh)
        self.image, self.mask = u8(*(shape + ((3,) if self.ch == 3 else ()))), u8(*shape)
        self.planes = [u8(*shape) for _ in range(st.extras)]
        self.counts = torch.full((8,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

    def __call__(self, images=None, M=None, o=None, k=None, cnt=None, window=None):
        st, kw = self.st, self.st.keywords(self.case)
        if window is not None:
            kw["window"] = window
        fn = getattr(self.s, st.name + "_frame_dev")
        lead = [self.images if images is None else images, self.ch, self.maps, self.Rs, self.ts, self.case["K"], self.rows, self.cols, self.M if M is None else M, self.m]
        lead += [self.case["weight"]] if st.name == "retime" else []
        outs = [self.image.data_ptr() if o is None else o, self.mask.data_ptr() if k is None else k] + [p.data_ptr() for p in self.planes]
        return fn(*lead, *outs, self.counts[1:].data_ptr() if cnt is None else cnt, *st.tail, **kw)

    def untouched(self):
        return all((x.cpu().numpy() == GUARD).all() for x in [self.image, self.mask] + self.planes) and self.counts.cpu().numpy().tolist() == [-1] * 8


@pytest.mark.parametrize("st", STAGES, ids=IDS)
def test_a_frame_call_says_what_it_refuses(oracle, rsdsfm, st):
    import torch

    text = FRAME_TEXT[st.name]
    case = st.case(oracle)
    with rsdsfm.Solver(0) as s:
        if isinstance(st, Medoid):
            s.set_plate_estimator(1)
        s.set_occlusion_search(case.get("search", 0))
        call = FrameCall(torch, s, st, case)
        nan_M = call.M.copy()
        nan_M.reshape(-1)[0] = np.nan
        with _null_argument(s.lib, "rsdsfm_%s_frame_dev" % st.name, 1):
            _refused(rsdsfm, call, text["null_array"], "null_array")
        for what, bad in (("null_source", dict(images=[0] + call.images[1:])), ("aliased_source", dict(images=[call.image.data_ptr()] + call.images[1:])),
                          ("nan_pose", dict(M=nan_M)), ("tall_window", dict(window=(0, 0, call.rows + 1, call.cols))), ("null_image", dict(o=0)),
                          ("mask_is_image", dict(k=call.image.data_ptr())), ("plane_plus_1", dict(o=call.image.data_ptr() + 1)),
                          ("counters_plus_4", dict(cnt=call.counts.data_ptr() + 4))):
            _refused(rsdsfm, lambda: call(**bad), text[what], what)
        s.synchronize()
        assert call.untouched()  # nothing was enqueued
        s.set_occlusion_search(0)
        st.check(torch, s, case)


def _accumulate_planes(torch, L=1):
    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    u8 = lambda value, *shape: torch.full(shape, value, dtype=torch.uint8, device=dev)
    p = dict(ref=u8(9, rows, cols, 3), rmask=u8(1, rows, cols), lay=[u8(9 + j, rows, cols, 3) for j in range(L)], lmask=[u8(1, rows, cols) for _ in range(L)],
             out=u8(GUARD, rows, cols, 3), omask=u8(GUARD, rows, cols), extra=[u8(GUARD, rows, cols), u8(GUARD, rows, cols)],
             cells=torch.full((rows, cols, 4), 0x7BCD, dtype=torch.int16, device=dev), counts=torch.full((6,), -1, dtype=torch.int64, device=dev),
             rec=torch.zeros(8 * L + 1, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    return rows, cols, p


def _output_faults(p):
    return (("null_image", dict(o=0)), ("mask_is_image", dict(k=p["out"].data_ptr())), ("plane_plus_1", dict(o=p["out"].data_ptr() + 1)),
            ("counters_plus_4", dict(cnt=p["counts"].data_ptr() + 4)))


def _input_faults(p):
    ref = p["ref"].data_ptr()
    return (("first_2", dict(first=2)), ("null_reference", dict(R=0)), ("null_layer_mask", dict(mL=0)), ("layer_is_reference", dict(L=ref)), ("null_cells", dict(cl=0, first=0)),
            ("reference_plus_1", dict(R=ref + 1)), ("record_plus_4", dict(rc=p["rec"].data_ptr() + 4)), ("image_is_reference", dict(o=ref)), ("cells_are_reference", dict(cl=ref)))


def _nothing_written(p):
    return all((x.cpu().numpy() == GUARD).all() for x in [p["out"], p["omask"]] + p["extra"]) and p["counts"].cpu().numpy().tolist() == [-1] * 6 and \
        (p["cells"].cpu().numpy().view(np.uint16) == 0x7BCD).all()


def test_the_denoise_accumulate_says_what_it_refuses(rsdsfm):
    import torch

    rows, cols, p = _accumulate_planes(torch)
    text = ACCUMULATE_TEXT["denoise"]
    with rsdsfm.Solver(0) as s:
        def acc(R=p["ref"].data_ptr(), mR=p["rmask"].data_ptr(), L=p["lay"][0].data_ptr(), mL=p["lmask"][0].data_ptr(), cl=p["cells"].data_ptr(), first=1, rc=p["rec"].data_ptr(),
                o=p["out"].data_ptr(), k=p["omask"].data_ptr(), cnt=p["counts"][1:].data_ptr()):
            return s.denoise_accumulate_dev(R, mR, L, mL, 3, rows, cols, cl, first, 1, rc, 0, 0, 12, o, k, p["extra"][0].data_ptr(), cnt)

        for what, bad in _output_faults(p) + _input_faults(p):
            _refused(rsdsfm, lambda: acc(**bad), text[what], what)
        s.synchronize()
        assert _nothing_written(p)
        acc()  # reference and layer 9 under full masks: the mean is 9, the weight 16 + 16
        s.synchronize()
        assert (p["out"].cpu().numpy() == 9).all() and (p["omask"].cpu().numpy() == 1).all() and (p["extra"][0].cpu().numpy() == 32).all()
        assert p["counts"].cpu().numpy().tolist() == [-1, 0, 0, rows * cols, -1, -1]


def test_the_deblur_accumulate_says_what_it_refuses(rsdsfm):
    import torch

    rows, cols, p = _accumulate_planes(torch)
    text = ACCUMULATE_TEXT["deblur"]
    sharp = torch.from_numpy(np.concatenate([deblur_cases.sharp_records()["cap"][0], [0]]).astype(np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        def acc(R=p["ref"].data_ptr(), mR=p["rmask"].data_ptr(), L=p["lay"][0].data_ptr(), mL=p["lmask"][0].data_ptr(), cl=p["cells"].data_ptr(), first=1, sh=sharp.data_ptr(),
                rc=p["rec"].data_ptr(), o=p["out"].data_ptr(), k=p["omask"].data_ptr(), cnt=p["counts"][1:].data_ptr()):
            return s.deblur_accumulate_dev(R, mR, L, mL, 3, rows, cols, cl, first, 1, sh, rc, 0, 0, 24, 0, 0, 0, o, k, p["extra"][0].data_ptr(), cnt)

        faults = _output_faults(p) + _input_faults(p) + (("null_sharpness", dict(sh=0)), ("record_plus_4", dict(sh=sharp.data_ptr() + 4)), ("cells_are_record", dict(cl=p["rec"].data_ptr())))
        for what, bad in faults:
            _refused(rsdsfm, lambda: acc(**bad), text[what], what)
        s.synchronize()
        assert _nothing_written(p)
        acc()  # tau at its cap, 32: the layer counts 16 + 32 beside the own frame's 16 -- tests/test_gpu_deblur.py's numbers
        s.synchronize()
        assert (p["out"].cpu().numpy() == 9).all() and (p["omask"].cpu().numpy() == 1).all() and (p["extra"][0].cpu().numpy() == 48).all()
        assert p["counts"].cpu().numpy().tolist() == [-1, 0, 0, rows * cols, -1, -1]


def test_the_superres_accumulate_says_what_it_refuses(rsdsfm):
    import torch

    rows, cols, p = _accumulate_planes(torch)
    text = ACCUMULATE_TEXT["superres"]
    dev = torch.device("cuda", 0)
    u8 = lambda value, *shape: torch.full(shape, value, dtype=torch.uint8, device=dev)
    rnear, rprox, lnear, lprox = u8(20, rows, cols, 3), u8(4, rows, cols), u8(40, rows, cols, 3), u8(12, rows, cols)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        def acc(o=p["out"].data_ptr(), k=p["omask"].data_ptr(), cnt=p["counts"][1:].data_ptr()):
            return s.superres_accumulate_dev(p["ref"].data_ptr(), rnear.data_ptr(), rprox.data_ptr(), p["lay"][0].data_ptr(), lnear.data_ptr(), lprox.data_ptr(), 3, rows, cols,
                                             p["cells"].data_ptr(), 1, 1, p["rec"].data_ptr(), 0, 0, 12, o, k, p["extra"][0].data_ptr(), cnt)

        for what, bad in _output_faults(p):
            _refused(rsdsfm, lambda: acc(**bad), text[what], what)
        s.synchronize()
        assert _nothing_written(p)
        acc()  # tests/test_gpu_superres.py's numbers: own nearest 20 at 4, the layer's nearest 40 at 12: (4 * 20 + 12 * 40) / 16 = 35
        s.synchronize()
        assert (p["out"].cpu().numpy() == 35).all() and (p["omask"].cpu().numpy() == 1).all() and (p["extra"][0].cpu().numpy() == 16).all()
        assert p["counts"].cpu().numpy().tolist() == [-1, 0, 0, rows * cols, -1, -1]


@pytest.mark.parametrize("estimator", ["median", "medoid"])
def test_the_plate_estimators_say_what_they_refuse(rsdsfm, estimator):
    import torch

    rows, cols, p = _accumulate_planes(torch, L=2)
    text = ACCUMULATE_TEXT["plate"]
    with rsdsfm.Solver(0) as s:
        fn = s.plate_median_dev if estimator == "median" else s.plate_medoid_dev

        def est(o=p["out"].data_ptr(), k=p["omask"].data_ptr(), cnt=p["counts"][1:].data_ptr()):
            return fn(p["ref"].data_ptr(), p["rmask"].data_ptr(), [x.data_ptr() for x in p["lay"]], [x.data_ptr() for x in p["lmask"]], 3, rows, cols, o, k,
                      p["extra"][0].data_ptr(), p["extra"][1].data_ptr(), cnt, p["rec"].data_ptr(), 0, 0, 24, 3)

        for what, bad in _output_faults(p):
            _refused(rsdsfm, lambda: est(**bad), text[what], what)
        _refused(rsdsfm, lambda: est(cnt=p["extra"][0].data_ptr()), COUNTERS_ARE_A_PLANE["plate"], "counters_are_a_plane")
        s.synchronize()
        assert _nothing_written(p)
        est()  # candidates 9, 9, 10 in every channel: the lower median and the medoid are 9, all three agree, nothing moves
        s.synchronize()
        assert (p["out"].cpu().numpy() == 9).all() and (p["omask"].cpu().numpy() == 1).all() and (p["extra"][0].cpu().numpy() == 3).all() and (p["extra"][1].cpu().numpy() == 1).all()
        assert p["counts"].cpu().numpy().tolist() == [-1, 0, rows * cols, 0, 0, -1]


@pytest.mark.parametrize("st", [x for x in STAGES if x.name in COUNTERS_ARE_A_PLANE and not isinstance(x, Medoid)], ids=lambda x: x.name)
def test_counters_that_are_an_output_plane(oracle, rsdsfm, st):
    """the difference the shared check keeps, call by call: the denoise, the deblur and the super-resolution accept counters that are their weight
    plane (the call goes through and enqueues), the plate and the erase refuse them with their "distinct" message and enqueue nothing"""
    import torch

    case = st.case(oracle)
    want = COUNTERS_ARE_A_PLANE[st.name]
    with rsdsfm.Solver(0) as s:
        s.set_occlusion_search(case.get("search", 0))
        call = FrameCall(torch, s, st, case)
        if want is None:
            call(cnt=call.planes[0].data_ptr())
            s.synchronize()
            assert not (call.image.cpu().numpy() == GUARD).all()
        else:
            _refused(rsdsfm, lambda: call(cnt=call.planes[0].data_ptr()), want, "counters_are_a_plane")
            s.synchronize()
            assert call.untouched()
        s.set_occlusion_search(0)
        st.check(torch, s, case)
