#!/usr/bin/env python3
"""Randomised GPU-vs-spec campaign of the stages behind the solve (not collected by pytest: run  python tests/fuzz_stages.py [cases] [seed]
on a GPU box; tests/test_gpu_stage_fuzz.py runs a slice of it, tests/test_stage_fuzz_cpu.py holds the generator to its promises without a GPU).

Case n of campaign `seed` is stage_fuzz_cases.random_case(n, seed): one of nine families -- flow check, link, depth fusion, dense rectifier,
stabilise, border fill, crop (the window search, then one frame through a window), seam (the distance, then one blended layer), inpaint --
at sides in [2, 300] biased to the tile edges, with strips both ways, 1 or 3 channels and parameters over the ranges the headers under
include/ document.  Every case goes through the DEVICE entry point with guard bytes behind every plane and is compared bit for bit with the
family's definition (tests/*_spec_numpy.py): in-out planes whole, read-only planes unchanged, optional outputs present and absent.  A drawn
parameter set the library rejects and a spec output that is not well defined are failures, never skips.

The campaign holds ONE Solver for its whole run, so the dense workspace (csrc/rectify_dense.hpp: DenseWs) is rebuilt at every change of size
and its lazily-created members are allocated in whatever order the draw produces.  Before every change of size a cheap probe (the inpainting
or the seam distance of a fixed mask, in turn) runs at the OLD size, and behind the first case at the new size at the NEW one: the first
time a probe runs it must equal its definition, every later time the same bytes.

Not covered: the second trip of the grid-stride loops whose grids are capped at 65536 blocks -- the warp kernels of the dense rectifier, the
stabiliser, the fill and the window frame, seam_distance_cols_kernel, the seam blend's kernels, inpaint_write_kernel and the
super-resolution's superres_warp_kernel (tests/fuzz_temporal.py draws that stage) take it only above 2^26 pixels, which no quick test
reaches.  (tests/test_gpu_stage_fuzz.py takes the two smaller caps, stabilize_count_kernel's and crop_search_kernel's, past one grid;
tests/test_gpu_temporal_fuzz.py retime_merge_kernel's and shutter_accumulate_kernel's.)  The clip calls are not driven either: they have their own "those calls one after another" tests.

Prints one line  FAIL seed ... case ...  per failing case with everything needed to rebuild it, then one line per differing output, and a
summary; returns 1 if anything failed.

Environment: FUZZ_ONLY=3,17 re-runs selected case numbers of a campaign (same cases / seed arguments)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stabilize_blend_spec_numpy as blend_spec  # noqa: E402
import stabilize_inpaint_cases as inpaint_cases  # noqa: E402
import stabilize_inpaint_spec_numpy as inpaint_spec  # noqa: E402
import stage_fuzz_cases as G  # noqa: E402
from test_gpu_stabilize_blend import GUARD, _blend, _distance, _guarded  # noqa: E402
from test_gpu_stabilize_crop import _window  # noqa: E402
from test_gpu_stabilize_inpaint import _frame  # noqa: E402

_SPEC = {}  # (seed, n) -> (case, inputs, the spec's outputs, what is not well defined): kept on request, for a second library build


def spec_of(n, seed, keep=False):
    import oracle_py

    if (seed, n) in _SPEC:
        return _SPEC[(seed, n)]
    case = G.random_case(n, seed)
    inp = G.inputs(case, oracle_py.pose_table)
    want = G.expected(case, inp)
    out = (case, inp, want, G.undefined(case, inp, want))
    if keep:
        _SPEC[(seed, n)] = out
    return out


# ---------------------------------------------------------------------------------------------------
# planes on the device
# ---------------------------------------------------------------------------------------------------
class _Planes:
    """the planes of one call, each with guard bytes behind it (_guarded): read-only ones are checked to be unchanged afterwards"""

    def __init__(self, torch):
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.guards, self.readonly = [], []

    def _put(self, a):
        a = np.ascontiguousarray(a)
        t, g = _guarded(self.torch, self.dev, a.view(np.uint8).reshape(-1))
        self.guards.append(g)
        return t

    def ro(self, name, a):
        t = self._put(a)
        self.readonly.append((name, t, np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        return t

    def rw(self, a):
        return self._put(a)

    def out(self, shape, dtype, fill):
        return self._put(np.full(shape, fill, dtype=dtype))

    def counter(self, fill=-7):
        """one int64 with a guard word on either side: pass .ptr, read .value()"""
        t = self._put(np.full(3, fill, dtype=np.int64))
        return _Counter(t, fill)

    def check(self, fails):
        for g in self.guards:
            if not (g.cpu().numpy() == GUARD).all():
                fails.append("guard bytes behind a plane were written")
                break
        for name, t, a in self.readonly:
            if not np.array_equal(t.cpu().numpy(), a):
                fails.append("read-only plane %s changed" % name)


class _Counter:
    def __init__(self, t, fill):
        self.t, self.fill, self.ptr = t, fill, t.data_ptr() + 8

    def value(self, fails, present=True):
        c = self.t.cpu().numpy().view(np.int64)
        if c[0] != self.fill or c[2] != self.fill or (not present and c[1] != self.fill):
            fails.append("a word next to the counter (or a counter that was not passed) was written: %r" % (c.tolist(),))
        return int(c[1])


def _host(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def _differ(fails, name, got, want):
    """bit for bit; a float plane is compared through its bit patterns"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        fails.append("%s: shape %s, expected %s" % (name, got.shape, want.shape))
        return
    g, w = got.view(np.uint8), want.view(np.uint8)
    if not np.array_equal(g, w):
        per = g.reshape(got.size, -1) != w.reshape(want.size, -1)
        where = np.flatnonzero(per.any(axis=1))
        fails.append("%s: %d of %d elements differ, the first at flat index %d (got %r, expected %r)" % (name, where.size, got.size, where[0], got.reshape(-1)[where[0]],
                                                                                                       want.reshape(-1)[where[0]]))


def _scalar(fails, name, got, want):
    if got != want:
        fails.append("%s: got %r, expected %r" % (name, got, want))


# ---------------------------------------------------------------------------------------------------
# one case per family
# ---------------------------------------------------------------------------------------------------
def _flow_check(torch, s, case, inp, want, fails):
    rows, cols, p = case.rows, case.cols, case.params
    P = _Planes(torch)
    in_place = p["in_place"] and "masked" not in p["without"]
    d_fwd = P.rw(inp["fwd"]) if in_place else P.ro("fwd", inp["fwd"])
    d_bwd = P.ro("bwd", inp["bwd"])
    mask = P.out((rows, cols), np.uint8, 77)
    masked = d_fwd if in_place else P.out((rows, cols, 2), np.float64, np.nan)
    resid, count = P.out((rows, cols), np.float64, np.nan), P.counter()
    torch.cuda.synchronize()
    ptr = lambda name, t: None if name in p["without"] else t.data_ptr()
    s.flow_consistency_dev(d_fwd.data_ptr(), d_bwd.data_ptr(), rows, cols, mask.data_ptr(), ptr("masked", masked), ptr("resid", resid),
                           None if "count" in p["without"] else count.ptr, a1=p["a1"], a2=p["a2"])
    s.synchronize()
    P.check(fails)
    _differ(fails, "mask", _host(mask, np.uint8, (rows, cols)), want["mask"])
    nan = lambda shape: np.full(shape, np.nan)
    _differ(fails, "masked", _host(masked, np.float64, (rows, cols, 2)), nan((rows, cols, 2)) if "masked" in p["without"] else want["masked"])
    _differ(fails, "resid", _host(resid, np.float64, (rows, cols)), nan((rows, cols)) if "resid" in p["without"] else want["resid"])
    got = count.value(fails, "count" not in p["without"])
    if "count" not in p["without"]:
        _scalar(fails, "count", got, want["count"])


def _link(torch, s, case, inp, want, fails):
    rows, cols, p = case.rows, case.cols, case.params
    P = _Planes(torch)
    d_f = [P.ro("field %d" % q, f) for q, f in enumerate(inp["fields"])]
    d_z = [P.ro("map %d" % q, np.asarray(z, dtype=np.float64).T) for q, z in enumerate(inp["maps"])]
    d_pl = [P.out((rows, cols), np.uint64, 0xCDCDCDCDCDCDCDCD) for _ in range(p["links"])] if p["own_planes"] else None
    torch.cuda.synchronize()
    ptrs = lambda ts: [t.data_ptr() for t in ts]
    rec = s.link_pairs_dev(ptrs(d_f), ptrs(d_z), inp["vs"], inp["ws"], inp["ks"], rows, cols, inp["K"], inp["gamma"], p["global_shutter"], ptrs(d_pl) if d_pl else None,
                           p["tol"], p["min_links"], p["radix_bits"])
    s.synchronize()
    P.check(fails)
    for q, w in enumerate(want["links"]):
        if d_pl:
            _differ(fails, "link %d ratio plane" % q, _host(d_pl[q], np.uint64, (rows, cols)), w["plane"])
        got = rec[q]
        _scalar(fails, "link %d (n, agree, valid)" % q, (got["n"], got["agree"], got["valid"]), (w["n"], w["agree"], w["valid"]))
        _scalar(fails, "link %d ratio (bits)" % q, "nan" if np.isnan(got["ratio"]) else hex(int(np.float64(got["ratio"]).view(np.uint64))),
                "nan" if w["n"] == 0 else hex(int(np.float64(w["ratio"]).view(np.uint64))))


def _fuse(torch, s, case, inp, want, fails):
    rows, cols, p = case.rows, case.cols, case.params
    n = p["pairs"]
    P = _Planes(torch)
    d_f = [P.ro("field %d" % q, f) for q, f in enumerate(inp["fields"])]
    d_z = [P.ro("map %d" % q, np.asarray(z, dtype=np.float64).T) for q, z in enumerate(inp["maps"])]
    d_out = [P.out((cols, rows), np.uint64, 0xCDCDCDCDCDCDCDCD) for _ in range(n)]
    d_fl = [P.out((rows, cols), np.uint8, 0xCD) for _ in range(n)] if p["flags"] else None
    d_pl = [P.out((rows, cols), np.uint64, 0xCDCDCDCDCDCDCDCD) for _ in range(n - 1)] if p["planes"] else None
    torch.cuda.synchronize()
    ptrs = lambda ts: [t.data_ptr() for t in ts] if ts is not None else None
    rec = s.fuse_depths_dev(ptrs(d_f), ptrs(d_z), inp["vs"], inp["ws"], inp["ks"], rows, cols, inp["K"], inp["gamma"], inp["records"], ptrs(d_out), p["global_shutter"],
                            ptrs(d_fl), ptrs(d_pl), p["tol"])
    s.synchronize()
    P.check(fails)
    for q in range(n):
        _differ(fails, "fused map %d" % q, _host(d_out[q], np.float64, (cols, rows)).T, np.asarray(want["fused"][q], dtype=np.float64))
        if d_fl:
            _differ(fails, "flags %d" % q, _host(d_fl[q], np.uint8, (rows, cols)), want["flags"][q])
        _scalar(fails, "record %d" % q, rec[q], want["records"][q])
    for l in range(n - 1 if d_pl else 0):
        _differ(fails, "splat plane %d" % l, _host(d_pl[l], np.uint64, (rows, cols)), want["splat"][l])


def _frame_inputs(P, case, inp):
    return (P.ro("image", inp["image"]).data_ptr(), case.channels, P.ro("depth map", np.asarray(inp["depth"], dtype=np.float64).T).data_ptr(),
            P.ro("pose table R", inp["R"]).data_ptr(), P.ro("pose table t", inp["t"]).data_ptr(), inp["K"], case.rows, case.cols)


def _dense_kw(p):
    return dict(mode=p["mode"], q5_mode=p["q5_mode"], iterations=p["iterations"])


def _dense_outputs(P, case, want, without=()):
    """the dense rectifier's and the stabiliser's outputs, prefilled: (image, mask, filled, disp) with None for an output that is not passed"""
    rows, cols = case.rows, case.cols
    disp_fill = np.nan if not np.isnan(want["disp"]).any() else 12345.0  # (NaN could not tell an unwritten pair from a NaN result)
    return (P.out(want["image"].shape, np.uint8, 77), None if "mask" in without else P.out((rows, cols), np.uint8, 77),
            None if "filled" in without else P.out((cols, rows), np.float64, np.nan), None if "disp" in without else P.out((rows, cols, 2), np.float32, disp_fill))


def _dense_compare(case, want, out, mask, filled, disp, fails):
    rows, cols = case.rows, case.cols
    _differ(fails, "image", _host(out, np.uint8, want["image"].shape), want["image"])
    if mask is not None:
        _differ(fails, "mask", _host(mask, np.uint8, (rows, cols)), want["mask"])
    if filled is not None:
        _differ(fails, "filled depth", _host(filled, np.float64, (cols, rows)).T, want["filled"])
    if disp is not None:  # where the definition's displacement is NaN the kernel's must be NaN (any NaN); everything else bit for bit
        got, nan = _host(disp, np.float32, (rows, cols, 2)), np.isnan(want["disp"])
        if not np.array_equal(np.isnan(got), nan):
            fails.append("displacement: NaN at other places")
        else:
            _differ(fails, "displacement", np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want["disp"]))


def _dense(torch, s, case, inp, want, fails):
    p = case.params
    P = _Planes(torch)
    head = _frame_inputs(P, case, inp)
    out, mask, filled, disp = _dense_outputs(P, case, want, p["without"])
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()
    s.rectify_dense_frame_dev(*head, out.data_ptr(), ptr(mask), ptr(filled), ptr(disp), **_dense_kw(p))
    s.synchronize()
    P.check(fails)
    _dense_compare(case, want, out, mask, filled, disp, fails)


def _stabilize(torch, s, case, inp, want, fails):
    p = case.params
    P = _Planes(torch)
    head = _frame_inputs(P, case, inp)
    out, mask, filled, disp = _dense_outputs(P, case, want)
    valid = P.counter()
    torch.cuda.synchronize()
    s.stabilize_frame_dev(*head, inp["M"], inp["m"], out.data_ptr(), mask.data_ptr(), filled.data_ptr(), disp.data_ptr(), valid.ptr if p["with_valid"] else None, **_dense_kw(p))
    s.synchronize()
    P.check(fails)
    _dense_compare(case, want, out, mask, filled, disp, fails)
    got = valid.value(fails, p["with_valid"])
    if p["with_valid"]:
        _scalar(fails, "valid", got, want["valid"])


def _inout_call(torch, s, case, inp, want, fails, window=None):
    """rsdsfm_stabilize_fill_frame_dev, or with a window rsdsfm_stabilize_window_frame_dev, on the case's starting planes"""
    rows, cols, p = case.rows, case.cols, case.params
    P = _Planes(torch)
    head = _frame_inputs(P, case, inp)
    start = inp["start"]
    image, mask, count = P.rw(start["image"]), P.rw(start["mask"]), P.counter()
    source = P.rw(start["source"]) if p["with_source"] else P.ro("source (not passed)", start["source"])
    tail = (image.data_ptr(), mask.data_ptr(), source.data_ptr() if p["with_source"] else None, count.ptr if p["with_count"] else None)
    torch.cuda.synchronize()
    if window is None:
        s.stabilize_fill_frame_dev(*head, inp["M"], inp["m"], p["sid"], *tail, **_dense_kw(p))
    else:
        s.stabilize_window_frame_dev(*head, inp["M"], inp["m"], p["sid"], window, *tail, **_dense_kw(p))
    s.synchronize()
    P.check(fails)
    _differ(fails, "image", _host(image, np.uint8, start["image"].shape), want["image"])
    _differ(fails, "mask", _host(mask, np.uint8, (rows, cols)), want["mask"])
    if p["with_source"]:
        _differ(fails, "source", _host(source, np.uint8, (rows, cols)), want["source"])
    got = count.value(fails, p["with_count"])
    if p["with_count"]:
        _scalar(fails, "count", got, want["count"])


def _fill(torch, s, case, inp, want, fails):
    _inout_call(torch, s, case, inp, want, fails)


def _asserting(fails, what, call):
    """the existing tests' helpers assert that guards and read-only planes are untouched"""
    try:
        return call()
    except AssertionError as e:
        fails.append("%s: guard bytes or a read-only plane were written (%s)" % (what, e))
        return None


def _crop(torch, s, case, inp, want, fails):
    p = case.params
    found = _asserting(fails, "window search", lambda: _window(torch, s, inp["masks"], p["max_empty"], p["margin"]))
    _scalar(fails, "window", found, want["found"])
    _inout_call(torch, s, case, inp, want, fails, window=want["window"])


def _seam(torch, s, case, inp, want, fails):
    p = case.params
    T = p["feather"]
    dist = _asserting(fails, "distance", lambda: _distance(torch, s, inp["mask"] if case.op == "distance" else inp["own"], T))
    if dist is not None:
        _differ(fails, "distance", dist, want["dist"])
    if case.op == "blend":
        got = _asserting(fails, "blend", lambda: _blend(torch, s, inp, T, sid=p["sid"], gain=p["gain"], min_overlap=p["min_overlap"], with_counts=p["with_counts"]))
        if got is not None:
            for k in ("image", "mask", "source", "sums"):
                _differ(fails, k, got[k], want[k])
            if p["with_counts"]:
                _scalar(fails, "counts (filled, blended)", got["counts"], want["counts"])


def _inpaint(torch, s, case, inp, want, fails):
    p = case.params
    got = _asserting(fails, "inpaint", lambda: _frame(torch, s, inp["image"], inp["mask"], p["with_source"], p["with_count"]))
    if got is not None:
        _differ(fails, "image", got[0], want["image"])
        if p["with_source"]:
            _differ(fails, "source", got[1], want["source"])
        if p["with_count"]:
            _scalar(fails, "count", got[2], want["count"])


RUN = dict(flow_check=_flow_check, link=_link, fuse=_fuse, dense=_dense, stabilize=_stabilize, fill=_fill, crop=_crop, seam=_seam, inpaint=_inpaint)


def check_case(torch, solver, case, inp, want):
    """-> list of failure strings (empty when the case is clean)"""
    fails = []
    RUN[case.family](torch, solver, case, inp, want, fails)
    return fails


# ---------------------------------------------------------------------------------------------------
# the probe around every change of size
# ---------------------------------------------------------------------------------------------------
class _Probe:
    """a cheap call repeated at a size the context has seen: the first time against its definition, afterwards the same bytes"""

    def __init__(self):
        self.first, self.turn = {}, 0

    def run(self, torch, s, shape):
        rows, cols = shape
        kind = ("inpaint", "distance")[self.turn % 2]
        self.turn += 1
        mask = inpaint_cases.masks(rows, cols, rows + 3 * cols)[3][1]
        if kind == "inpaint":
            image = inpaint_cases.image_of(rows, cols, 1, 13 * rows + cols)
            out, src, count = _frame(torch, s, image, mask)
            got = out.tobytes() + src.tobytes() + bytes([count % 251])
        else:
            got = _distance(torch, s, mask, 8).tobytes()
        key = (kind, shape)
        if key not in self.first:
            if kind == "inpaint":
                want, want_src = image.copy(), np.zeros_like(mask)
                n = inpaint_spec.inpaint(want, mask, want_src)
                self.first[key] = want.tobytes() + want_src.tobytes() + bytes([n % 251])
            else:
                self.first[key] = blend_spec.seam_distance(mask, 8).tobytes()
            return [] if got == self.first[key] else ["probe (%s at %dx%d) differs from its definition" % (kind, rows, cols)]
        return [] if got == self.first[key] else ["probe (%s at %dx%d) no longer gives the bytes it gave the first time" % (kind, rows, cols)]


def main(cases=None, seed=None, arith="reference", keep_specs=False):
    import torch

    import rsdsfm

    if isinstance(cases, (list, tuple)):  # selected case numbers (tests/test_gpu_stage_fuzz.py::test_regressions)
        todo, seed = list(cases), seed or 1
    else:
        cases = int(sys.argv[1]) if cases is None and len(sys.argv) > 1 else (cases or 100)
        seed = int(sys.argv[2]) if seed is None and len(sys.argv) > 2 else (seed or 1)
        todo = [int(x) for x in os.environ.get("FUZZ_ONLY", "").split(",") if x] or list(range(cases))
    bad, size, probe, stopped = 0, None, _Probe(), False
    with rsdsfm.Solver(0, arith=arith) as s:
        for n in todo:
            case, inp, want, undefined = spec_of(n, seed, keep_specs)
            shape = (case.rows, case.cols)
            fails = ["the SPEC is not well defined: " + u for u in undefined]
            try:
                if size is not None and shape != size:
                    fails += ["before the change of size: " + f for f in probe.run(torch, s, size)]
                fails += check_case(torch, s, case, inp, want)
                if shape != size:
                    fails += ["after the change of size: " + f for f in probe.run(torch, s, shape)]
            except AssertionError as e:  # a helper's own check of guards and read-only planes
                fails.append("AssertionError: %s" % (e,))
            except Exception as e:  # a rejected call is a failure too: every drawn parameter set is a documented one
                fails.append("%s: %s" % (type(e).__name__, e))
                fails.append("stopping here: after an error of the library or the runtime nothing more is started on the GPU")
                stopped = True
            size = shape
            if fails:
                bad += 1
                print("FAIL seed %d case %d (%s): %s" % (seed, n, arith, G.describe(case)))
                for f in fails:
                    print("    " + f)
            if stopped:
                break
    print("fuzz_stages: %d cases (seed %d, %s), %d failed" % (len(todo), seed, arith, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
