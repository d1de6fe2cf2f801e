#!/usr/bin/env python3
"""Randomised GPU-vs-spec campaign of the temporal image stages (not collected by pytest: run  python tests/fuzz_temporal.py [cases] [seed]  on a
GPU box; tests/test_gpu_temporal_fuzz.py runs a slice of it, tests/test_temporal_fuzz_cpu.py holds the generator to its promises without a GPU).

Case n of campaign `seed` is temporal_fuzz_cases.random_case(n, seed): the retimer's merge, the shutter's, the denoise's and the
super-resolution's accumulate chains, the blend's record as a call, the super-resolution's render, the plate's median -- on caller-owned
planes -- and the five frame calls on the context's workspace, with the keywords the helpers of
tests/test_gpu_{retime,shutter,denoise,superres,plate}.py build.  Every caller plane lies at a drawn byte offset of the MINIMUM alignment the
headers admit (4 bytes for byte planes, 8 for cells, records and counters; depth maps and pose tables stay at 0, the device API's 16-byte rule;
the buffers themselves are checked to start on 16), with guard bytes in front of it and behind it.
Everything is compared bit for bit with the definition (tests/*_spec_numpy.py): outputs whole, the chains' cells whole before the last step
(so a mid step that touches a cell under an empty word shows) and unchanged behind it, read-only planes unchanged, outputs and counters that
were not passed untouched.  A drawn parameter set the library rejects and a spec output that is not well defined are failures, never skips.

About one case in four is a case of the EXISTING campaign (tests/fuzz_stages.py: check_case), run on the same Solver: blend, crop and inpaint
calls fall between retime, denoise and plate calls on the shared layer and workspace, the plate's stack grows and shrinks and the
super-resolution's scale changes in whatever order the draw produces.  Before every change of the frame size of the workspace's users (the
frame calls and the existing campaign's cases) a cheap probe -- a two-source retime frame and a three-source plate frame, in turn -- runs at
the OLD size, and behind the first case at the new size at the NEW one: the first time a probe runs it must equal its definition, every later
time the same bytes.

Not covered: the clip calls (they have their "frame calls one after another" tests) and superres_warp_kernel's second trip (65536 blocks).
tests/test_gpu_temporal_fuzz.py takes retime_merge_kernel's and shutter_accumulate_kernel's loops past one grid.

The run ends at once, with no further launch, when a call returns anything but a refusal of its arguments or a synchronize fails.

Prints one line  FAIL seed ... case ...  per failing case with everything needed to rebuild it, then one line per differing output, a summary
and the counts per family; returns 1 if anything failed.

Environment: FUZZ_ONLY=3,17 re-runs selected case numbers of a campaign (same cases / seed arguments)."""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import denoise_cases as dcases  # noqa: E402
import fuzz_stages  # noqa: E402
import plate_cases as pcases  # noqa: E402
import retime_cases as rcases  # noqa: E402
import shutter_cases as scases  # noqa: E402
import temporal_fuzz_cases as T  # noqa: E402
from fuzz_stages import _differ, _scalar  # noqa: E402
from test_gpu_denoise import _frame_kw as denoise_frame_kw  # noqa: E402
from test_gpu_plate import _frame as plate_frame  # noqa: E402
from test_gpu_plate import _frame_kw as plate_frame_kw  # noqa: E402
from test_gpu_retime import _frame as retime_frame  # noqa: E402
from test_gpu_shutter import _render_kw as shutter_render_kw  # noqa: E402
from test_gpu_superres import _frame_kw as superres_frame_kw  # noqa: E402

GUARD = 0xCD
FRONT, BACK = 16, 16  # guard bytes in front of a plane (before its drawn offset) and behind it
_SPEC = {}  # (seed, n) -> (case, inputs, the spec's outputs, what is not well defined): kept on request, for a second library build
_PROBE_SPEC = {}


def spec_of(n, seed, keep=False):
    import oracle_py

    if (seed, n) in _SPEC:
        return _SPEC[(seed, n)]
    case = T.random_case(n, seed)
    inp = T.inputs(case, oracle_py.pose_table)
    want = T.expected(case, inp)
    out = (case, inp, want, T.undefined(case, inp, want))
    if keep:
        _SPEC[(seed, n)] = out
    return out


# ---------------------------------------------------------------------------------------------------
# placed planes
# ---------------------------------------------------------------------------------------------------
class _Plane:
    def __init__(self, buf, lo, size):
        self.buf, self.lo, self.size, self.ptr = buf, lo, size, buf.data_ptr() + lo

    def host(self, dtype=np.uint8, shape=(-1,)):
        return self.buf[self.lo:self.lo + self.size].cpu().numpy().view(dtype).reshape(shape)

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:self.lo] == GUARD).all() and (b[self.lo + self.size:] == GUARD).all())


class _Placed:
    """the planes of one case: each in a buffer of its own that starts on 16 bytes, at FRONT + a drawn offset, GUARD bytes before and behind"""

    def __init__(self, torch, place):
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self._plane, self._cell = itertools.cycle(place["planes"]), itertools.cycle(place["cells"])
        self.all, self.readonly, self.untouched = [], [], []

    def _put(self, a, off):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        buf = self.torch.full((FRONT + off + b.size + BACK,), GUARD, dtype=self.torch.uint8, device=self.dev)
        assert buf.data_ptr() % 16 == 0, "the buffer does not start on 16 bytes: the residue would not be the drawn one"
        buf[FRONT + off:FRONT + off + b.size] = self.torch.from_numpy(b.copy()).to(self.dev)
        self.all.append(_Plane(buf, FRONT + off, b.size))
        return self.all[-1]

    def ro(self, name, a, kind="plane"):
        """a read-only plane; kind "cell": 8-byte data (a record), "fixed": offset 0 (depth maps and pose tables: the API's 16-byte rule)"""
        pl = self._put(a, dict(plane=lambda: next(self._plane), cell=lambda: next(self._cell), fixed=lambda: 0)[kind]())
        self.readonly.append((name, pl, np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        return pl

    def out(self, shape, passed=True, name="output"):
        """an output plane, never preset: every byte GUARD; not passed: it must stay so"""
        pl = self._put(np.full(shape, GUARD, dtype=np.uint8), next(self._plane))
        if not passed:
            self.untouched.append((name, pl))
        return pl

    def cells(self, a):
        return self._put(a, next(self._cell))

    def counter(self, k, passed=True, fill=-7):
        return _Counters(self._put(np.full(k + 2, fill, dtype=np.int64), next(self._cell)), k, fill, passed)

    def check(self, fails):
        if not all(pl.guards_intact() for pl in self.all):
            fails.append("guard bytes in front of or behind a plane were written")
        for name, pl, a in self.readonly:
            if not np.array_equal(pl.host(), a):
                fails.append("read-only plane %s changed" % name)
        for name, pl in self.untouched:
            if not (pl.host() == GUARD).all():
                fails.append("%s was not passed and was written" % name)


class _Counters:
    """k int64 with a guard word on either side"""

    def __init__(self, plane, k, fill, passed):
        self.plane, self.k, self.fill, self.passed, self.ptr = plane, k, fill, passed, plane.ptr + 8

    def arg(self):
        return self.ptr if self.passed else None

    def values(self, fails):
        c = self.plane.host(np.int64).tolist()
        if c[0] != self.fill or c[-1] != self.fill or (not self.passed and c[1:-1] != [self.fill] * self.k):
            fails.append("a word next to the counters (or counters that were not passed) was written: %r" % (c,))
        return c[1:-1]


def _garbage_cells(rows, cols, ch):
    """what `first` must not read: no two neighbouring values equal, none of them a sum the chain can reach"""
    return (60000 + (np.arange(rows * cols * (ch + 1)) * 7) % 5000).astype(np.uint16).reshape(rows, cols, ch + 1)


def _image_shape(rows, cols, ch):
    return (rows, cols) if ch == 1 else (rows, cols, 3)


def _compare_planes(fails, want, **planes):
    for k, (pl, shape) in planes.items():
        _differ(fails, k, pl.host(np.uint8, shape), want[k])


# ---------------------------------------------------------------------------------------------------
# the primitives
# ---------------------------------------------------------------------------------------------------
def _merge(torch, s, case, inp, want, fails):
    import rsdsfm

    rows, cols, ch, p = case.rows, case.cols, case.channels, case.params
    P = _Placed(torch, case.place)
    a, ka = P.ro("image a", inp["ia"]), P.ro("mask a", inp["ma"])
    b, kb = (P.ro("image b", inp["ib"]), P.ro("mask b", inp["mb"])) if p["b"] else (None, None)
    refused = bool(want.get("refused"))
    out, mask = P.out(inp["ia"].shape, not refused, "image"), P.out((rows, cols), not refused, "mask")
    source, cnt = P.out((rows, cols), p["with_source"] and not refused, "source"), P.counter(5, p["with_counts"])
    torch.cuda.synchronize()
    call = lambda: s.retime_merge_dev(a.ptr, ka.ptr, b.ptr if b else None, kb.ptr if kb else None, ch, rows, cols, p["weight"], out.ptr, mask.ptr,
                                      source.ptr if p["with_source"] else None, cnt.arg(), threshold=p["threshold"])
    if refused:
        try:
            call()
            fails.append("weight %d was not refused" % p["weight"])
        except rsdsfm.RsdsfmError as e:
            if "(-1)" not in str(e):
                raise
        s.synchronize()
        cnt.passed = False  # nothing was enqueued: the counters too keep their fill
        cnt.values(fails)
        P.check(fails)
        return
    call()
    s.synchronize()
    P.check(fails)
    _compare_planes(fails, want, image=(out, inp["ia"].shape), mask=(mask, (rows, cols)))
    if p["with_source"]:
        _compare_planes(fails, want, source=(source, (rows, cols)))
    got = cnt.values(fails)
    if p["with_counts"]:
        _scalar(fails, "counts", got, want["counts"])


def _chain_outputs(P, shape, plane_shape, with_third, with_counts, third):
    return P.out(shape), P.out(plane_shape), P.out(plane_shape, with_third, third), P.counter(3, with_counts)


def _cells_step(s, fails, cells, shape, want_cells, outs, what):
    """before the chain's last launch: the cells whole against the definition's, and the outputs still untouched"""
    s.synchronize()
    _differ(fails, "cells %s" % what, cells.host(np.uint16, shape), want_cells)
    if not all((pl.host() == GUARD).all() for pl in outs):
        fails.append("an output plane was written by a step that is not the last")


def _chain_compare(fails, P, cells, cells_shape, want_cells, want, image, mask, third, third_key, cnt, shape, plane_shape, with_third, with_counts):
    P.check(fails)
    _differ(fails, "cells behind the last step", cells.host(np.uint16, cells_shape), want_cells)
    _compare_planes(fails, want, image=(image, shape), mask=(mask, plane_shape))
    if with_third:
        _compare_planes(fails, want, **{third_key: (third, plane_shape)})
    got = cnt.values(fails)
    if with_counts:
        _scalar(fails, "counts", got, want["counts"])


def _shutter(torch, s, case, inp, want, fails):
    rows, cols, ch, p = case.rows, case.cols, case.channels, case.params
    S, shape = p["S"], _image_shape(rows, cols, ch)
    P = _Placed(torch, case.place)
    d = [(P.ro("sample %d" % j, i), P.ro("sample mask %d" % j, m)) for j, (i, m) in enumerate(inp["samples"])]
    garbage = _garbage_cells(rows, cols, ch)
    cells = P.cells(garbage)
    image, mask, cov, cnt = _chain_outputs(P, shape, (rows, cols), p["with_coverage"], p["with_counts"], "coverage")
    want_cells = garbage if want["cells_before"] is None else want["cells_before"]
    torch.cuda.synchronize()
    for j, (d_i, d_m) in enumerate(d):
        if j == S - 1:
            _cells_step(s, fails, cells, garbage.shape, want_cells, (image, mask, cov), "before the last sample")
        s.shutter_accumulate_dev(d_i.ptr, d_m.ptr, ch, rows, cols, cells.ptr, j == 0, j == S - 1, S, p["min_samples"], image.ptr, mask.ptr,
                                 cov.ptr if p["with_coverage"] else None, cnt.arg())
    s.synchronize()
    _chain_compare(fails, P, cells, garbage.shape, want_cells, want, image, mask, cov, "coverage", cnt, shape, (rows, cols), p["with_coverage"], p["with_counts"])


def _sums(torch, s, case, inp, want, fails):
    rows, cols, ch = case.rows, case.cols, case.channels
    P = _Placed(torch, case.place)
    d = [P.ro(k, inp[k]) for k in ("image", "source", "layer", "lmask")]
    rec = P.counter(8)
    torch.cuda.synchronize()
    s.seam_overlap_sums_dev(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, ch, rows, cols, rec.ptr)
    s.synchronize()
    P.check(fails)
    _scalar(fails, "sums", rec.values(fails), np.asarray(want["sums"], dtype=np.uint64).view(np.int64).tolist())


def _accumulate_chain(torch, s, case, inp, want, fails, superres):
    """the denoise's chain, or the super-resolution's on its three planes per layer"""
    rows, cols, ch, p = case.rows, case.cols, case.channels, case.params
    L, shape = p["L"], _image_shape(rows, cols, ch)
    P = _Placed(torch, case.place)
    keys = ("ref", "near", "prox") if superres else ("ref", "rmask")
    ref = [P.ro(k, inp[k]) for k in keys]
    d_l = [[P.ro("layer %d plane %d" % (j, i), a) for i, a in enumerate(layer)] for j, layer in enumerate(inp["layers"])]
    d_rec = [None if inp["records"] is None or inp["records"][j] is None else P.ro("record %d" % j, np.asarray(inp["records"][j], dtype=np.uint64), "cell") for j in range(L)]
    garbage = _garbage_cells(rows, cols, ch)
    cells = P.cells(garbage)
    image, mask, weight, cnt = _chain_outputs(P, shape, (rows, cols), p["with_weight"], p["with_counts"], "weight")
    want_cells = garbage if want["cells_before"] is None else want["cells_before"]
    call = s.superres_accumulate_dev if superres else s.denoise_accumulate_dev
    kw = dict(min_overlap=p["min_overlap"], gain_mode=p["gain_mode"], strength=p["strength"], d_image_out=image.ptr, d_mask_out=mask.ptr,
              d_weight=weight.ptr if p["with_weight"] else None, d_counts3=cnt.arg())
    torch.cuda.synchronize()
    if L == 0:  # first and last, no layer: the cells may be passed and are neither read nor written
        call(*[r.ptr for r in ref], *[None] * len(keys), ch, rows, cols, cells.ptr, True, True, **kw)
    for j, dl in enumerate(d_l):
        if j == L - 1:
            _cells_step(s, fails, cells, garbage.shape, want_cells, (image, mask, weight), "before the last layer")
        call(*[r.ptr for r in ref], *[x.ptr for x in dl], ch, rows, cols, cells.ptr, j == 0, j == L - 1, d_sums8=d_rec[j].ptr if d_rec[j] else None, **kw)
    s.synchronize()
    _chain_compare(fails, P, cells, garbage.shape, want_cells, want, image, mask, weight, "weight", cnt, shape, (rows, cols), p["with_weight"], p["with_counts"])


def _denoise(torch, s, case, inp, want, fails):
    _accumulate_chain(torch, s, case, inp, want, fails, False)


def _superres_accumulate(torch, s, case, inp, want, fails):
    _accumulate_chain(torch, s, case, inp, want, fails, True)


def _superres_render(torch, s, case, inp, want, fails):
    rows, cols, ch, p = case.rows, case.cols, case.channels, case.params
    fine = (p["scale"] * rows, p["scale"] * cols)
    shape = fine + inp["image"].shape[2:]
    P = _Placed(torch, case.place)
    img = P.ro("image", inp["image"])
    z = P.ro("depth map", np.asarray(inp["depth"], dtype=np.float64).T, "fixed")
    R, t = P.ro("pose table R", np.asarray(inp["R"], dtype=np.float64).reshape(-1, 9), "fixed"), P.ro("pose table t", np.asarray(inp["t"], dtype=np.float64), "fixed")
    bil, near, prox, valid = P.out(shape), P.out(shape), P.out(fine), P.out(fine, p["with_valid"], "validity")
    torch.cuda.synchronize()
    s.superres_render_dev(img.ptr, ch, z.ptr, R.ptr, t.ptr, inp["K"], rows, cols, inp["M"], inp["m"], p["scale"], bil.ptr, near.ptr, prox.ptr,
                          valid.ptr if p["with_valid"] else None, p["window"], mode=p["mode"], q5_mode=p["q5_mode"], iterations=p["iterations"])
    s.synchronize()
    P.check(fails)
    _compare_planes(fails, want, bil=(bil, shape), near=(near, shape), prox=(prox, fine))
    if p["with_valid"]:
        _differ(fails, "validity", valid.host(np.uint8, fine), (want["prox"] != 0).astype(np.uint8))


def _plate(torch, s, case, inp, want, fails):
    rows, cols, ch, p = case.rows, case.cols, case.channels, case.params
    shape = _image_shape(rows, cols, ch)
    P = _Placed(torch, case.place)
    ref, rm = P.ro("ref", inp["ref"]), P.ro("ref mask", inp["rmask"])
    d_l = [(P.ro("layer %d" % j, i), P.ro("layer mask %d" % j, m)) for j, (i, m) in enumerate(inp["layers"])]
    rec = None if inp["records"] is None else P.ro("records", np.asarray(inp["records"], dtype=np.uint64), "cell")
    image, mask = P.out(shape), P.out((rows, cols))
    votes, moving, cnt = P.out((rows, cols), p["with_votes"], "votes"), P.out((rows, cols), p["with_moving"], "flag plane"), P.counter(4, p["with_counts"])
    torch.cuda.synchronize()
    s.plate_median_dev(ref.ptr, rm.ptr, [i.ptr for i, _ in d_l], [m.ptr for _, m in d_l], ch, rows, cols, image.ptr, mask.ptr, votes.ptr if p["with_votes"] else None,
                       moving.ptr if p["with_moving"] else None, cnt.arg(), rec.ptr if rec else None, min_overlap=p["min_overlap"], gain_mode=p["gain_mode"],
                       threshold=p["threshold"], min_votes=p["min_votes"])
    s.synchronize()
    P.check(fails)
    _compare_planes(fails, want, image=(image, shape), mask=(mask, (rows, cols)))
    for key, pl, passed in (("votes", votes, p["with_votes"]), ("moving", moving, p["with_moving"])):
        if passed:
            _compare_planes(fails, want, **{key: (pl, (rows, cols))})
    got = cnt.values(fails)
    if p["with_counts"]:
        _scalar(fails, "counts", got, want["counts"])


# ---------------------------------------------------------------------------------------------------
# the frame calls: the stages' own keyword builders, the planes placed here
# ---------------------------------------------------------------------------------------------------
OPTIONAL = dict(retime_frame=(("source", "with_source"),), shutter_frame=(("coverage", "with_coverage"),), denoise_frame=(("weight", "with_weight"),),
                superres_frame=(("weight", "with_weight"),), plate_frame=(("votes", "with_weight"), ("moving", "with_moving")))
COUNTERS = dict(retime_frame=5, shutter_frame=3, denoise_frame=3, superres_frame=3, plate_frame=4)


def _frame(torch, s, case, inp, want, fails):
    """one frame call of the case's family: images and outputs at drawn offsets, depth maps and pose tables at 0, the context's knob set to the
    case's for the call"""
    c, p, f = inp["case"], case.params, case.family
    rows, cols, ch = case.rows, case.cols, case.channels
    frames = c["images"] if f == "retime_frame" else c["frames"]
    if f in ("retime_frame", "shutter_frame"):
        src = list(range(len(frames)))
    else:
        src, M, m = dcases.sources_and_poses(c)
    P = _Placed(torch, case.place)
    f64 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    d = {n: (P.ro("image %d" % n, frames[n]), P.ro("depth map %d" % n, f64(c["depths"][n]).T, "fixed"), P.ro("pose table R %d" % n, f64(c["Rs"][n]).reshape(-1, 9), "fixed"),
             P.ro("pose table t %d" % n, f64(c["ts"][n]), "fixed")) for n in dict.fromkeys(src)}
    pick = lambda i: [d[n][i].ptr for n in src]
    scale = p["scale"] if f == "superres_frame" else 1
    fine = (scale * rows, scale * cols)
    shape = fine + frames[0].shape[2:]
    image, mask = P.out(shape), P.out(fine)
    optional = [(key, P.out(fine, p[flag], key), p[flag]) for key, flag in OPTIONAL[f]]
    cnt = P.counter(COUNTERS[f], p["with_counts"])
    tail = [image.ptr, mask.ptr] + [pl.ptr if passed else None for _, pl, passed in optional] + [cnt.arg()]
    torch.cuda.synchronize()
    s.set_occlusion_search(c["search"])
    try:
        if f == "retime_frame":
            s.retime_frame_dev(pick(0), ch, pick(1), pick(2), pick(3), c["K"], rows, cols, c["M"], c["m"], c["weight"], *tail, **shutter_render_kw(c))
        elif f == "shutter_frame":
            kept = s.shutter_frame_dev(pick(0), rows, cols, ch, c["K"], pick(1), pick(2), pick(3), c["A"], c["c"], c["A_path"], c["c_path"], c["scales"], c["t"], *tail,
                                       shutter=c["shutter"], samples=c["samples"], min_samples=c["min_samples"], **shutter_render_kw(c))
            _scalar(fails, "kept sub-instants", kept, len(want["times"]))
        else:
            call, kw = dict(denoise_frame=(s.denoise_frame_dev, denoise_frame_kw), superres_frame=(s.superres_frame_dev, superres_frame_kw),
                            plate_frame=(s.plate_frame_dev, plate_frame_kw))[f]
            call(pick(0), ch, pick(1), pick(2), pick(3), c["K"], rows, cols, M, m, *tail, **kw(c))
        s.synchronize()
    finally:
        s.set_occlusion_search(0)
    P.check(fails)
    _compare_planes(fails, want, image=(image, shape), mask=(mask, fine))
    for key, pl, passed in optional:
        if passed:
            _compare_planes(fails, want, **{key: (pl, fine)})
    got = cnt.values(fails)
    if p["with_counts"]:
        _scalar(fails, "counts", got, list(want["counts"]))


def _stage(torch, s, case, inp, want, fails):
    fails += fuzz_stages.check_case(torch, s, case.stage, inp, want)


RUN = dict(merge=_merge, shutter=_shutter, sums=_sums, denoise=_denoise, superres_render=_superres_render, superres_accumulate=_superres_accumulate, plate=_plate,
           retime_frame=_frame, shutter_frame=_frame, denoise_frame=_frame, superres_frame=_frame, plate_frame=_frame, stage=_stage)
WORKSPACE_USERS = T.FRAMES + ("stage",)  # the cases whose calls size the context's workspace


def check_case(torch, solver, case, inp, want):
    """-> list of failure strings (empty when the case is clean)"""
    fails = []
    RUN[case.family](torch, solver, case, inp, want, fails)
    return fails


# ---------------------------------------------------------------------------------------------------
# the probe around every change of size
# ---------------------------------------------------------------------------------------------------
def probe_case(kind, shape):
    """the fixed cheap call at a frame size: a two-source retime frame, or a three-source plate frame (gray)"""
    rows, cols = shape
    if kind == "retime":
        return rcases.smooth_pair(rows, cols, 1, 13 * rows + cols, 30000)
    clip = scases.smooth_clip(rows, cols, 1, rows + 3 * cols, t=0.0, shutter=0.0, samples=1, nsources=3)
    return dict(dcases.from_shutter(clip, "probe", 1, radius=1), threshold=24, min_votes=2)


def _probe_bytes(r, keys):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in keys) + repr(list(r["counts"])).encode()


def probe_spec(kind, shape):
    if (kind, shape) not in _PROBE_SPEC:
        case = probe_case(kind, shape)
        _PROBE_SPEC[(kind, shape)] = _probe_bytes(rcases.run_spec(case), ("image", "mask", "source")) if kind == "retime" else \
            _probe_bytes(pcases.run_spec(case), ("image", "mask", "votes", "moving"))
    return _PROBE_SPEC[(kind, shape)]


class _Probe:
    """a cheap call repeated at a size the context has seen: the first time against its definition, afterwards the same bytes"""

    def __init__(self):
        self.first, self.turn = {}, 0

    def run(self, torch, s, shape):
        kind = ("retime", "plate")[self.turn % 2]
        self.turn += 1
        case = probe_case(kind, shape)
        got = _probe_bytes(retime_frame(torch, s, case), ("image", "mask", "source")) if kind == "retime" else \
            _probe_bytes(plate_frame(torch, s, case), ("image", "mask", "votes", "moving"))
        key = (kind, shape)
        if key not in self.first:
            self.first[key] = got
            return [] if got == probe_spec(kind, shape) else ["probe (%s at %dx%d) differs from its definition" % (kind, shape[0], shape[1])]
        return [] if got == self.first[key] else ["probe (%s at %dx%d) no longer gives the bytes it gave the first time" % (kind, shape[0], shape[1])]


def main(cases=None, seed=None, arith="reference", keep_specs=False):
    import torch

    import rsdsfm

    if isinstance(cases, (list, tuple)):  # selected case numbers (tests/test_gpu_temporal_fuzz.py::test_regressions)
        todo, seed = list(cases), seed or 1
    else:
        cases = int(sys.argv[1]) if cases is None and len(sys.argv) > 1 else (cases or 100)
        seed = int(sys.argv[2]) if seed is None and len(sys.argv) > 2 else (seed or 1)
        todo = [int(x) for x in os.environ.get("FUZZ_ONLY", "").split(",") if x] or list(range(cases))
    bad, size, probe, stopped, ran, failed = 0, None, _Probe(), False, {}, {}
    with rsdsfm.Solver(0, arith=arith) as s:
        for n in todo:
            case, inp, want, undefined = spec_of(n, seed, keep_specs)
            shape = (case.rows, case.cols) if case.family in WORKSPACE_USERS else size
            fails = ["the SPEC is not well defined: " + u for u in undefined]
            try:
                if size is not None and shape != size:
                    fails += ["before the change of size: " + f for f in probe.run(torch, s, size)]
                fails += check_case(torch, s, case, inp, want)
                if shape != size:
                    fails += ["after the change of size: " + f for f in probe.run(torch, s, shape)]
            except AssertionError as e:  # a helper's own check of guards and read-only planes
                fails.append("AssertionError: %s" % (e,))
            except rsdsfm.RsdsfmError as e:  # a rejected call is a failure too: every drawn parameter set is a documented one
                fails.append("RsdsfmError: %s" % (e,))
                stopped = "(-1)" not in str(e)  # a refusal enqueues nothing; anything else (a HIP error) ends the run
            except Exception as e:
                fails.append("%s: %s" % (type(e).__name__, e))
                stopped = True
            if stopped:
                fails.append("stopping here: after an error of the library or the runtime nothing more is started on the GPU")
            size = shape
            name = case.family if case.family != "stage" else "stage/" + case.op
            ran[name] = ran.get(name, 0) + 1
            if fails:
                bad += 1
                failed[name] = failed.get(name, 0) + 1
                print("FAIL seed %d case %d (%s): %s" % (seed, n, arith, T.describe(case)))
                for f in fails:
                    print("    " + f)
            if stopped:
                break
    print("fuzz_temporal: %d cases (seed %d, %s), %d failed" % (len(todo), seed, arith, bad))
    print("    per family (failed / run): " + ", ".join("%s %d/%d" % (k, failed.get(k, 0), ran[k]) for k in sorted(ran)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
