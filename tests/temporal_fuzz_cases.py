"""The generator of the temporal image stages' randomised campaign (tests/fuzz_temporal.py on the GPU, tests/test_temporal_fuzz_cpu.py here), beside
tests/stage_fuzz_cases.py and with its contract: case n of campaign `seed` is random_case(n, seed), a record of plain Python values that depends
on nothing but (n, seed); inputs(case, pose_table) builds its arrays with the builders of the stages' own tests/*_cases.py modules,
expected(case, inp) runs the stage's definition (tests/*_spec_numpy.py), undefined(case, inp, want) names the outputs that are not well defined
(a failure of the generator, never a skip) and trivial(case, inp, want) says whether the definition's own output is one a kernel that does
nothing would also give.

Families (drawn, not dealt in turn).  Primitives on caller-owned planes, 1 or 3 channels: merge, shutter (a chain of accumulates), sums (the
blend's record as a call), denoise (a chain), superres_render, superres_accumulate (a chain), plate.  Frame calls on the context's workspace:
retime_frame, shutter_frame, denoise_frame, superres_frame, plate_frame.  About one case in four (STAGE_SHARE) is family "stage": case n of the
EXISTING campaign (stage_fuzz_cases.random_case(n, seed), unchanged), so that on one context its calls fall between these.

Sizes: the primitives take stage_fuzz_cases._size -- sides in [2, 300] biased to the tile edges, rows * cols <= 90000, strips of STRIP_LONG by
[2, 8]; the tile families (denoise, superres_accumulate, plate: 16 x 64 tiles whose edges lie along a row, 33 tiles across at 2050 columns)
draw strips, and wide ones, as often as that module's seam family.  superres_render's FINE grid counts against the 90000.  The frame calls stay
within 70 x 140, and nsrc * scale^2 * rows * cols within FRAME_WORK, for the definitions' time; their clips are the shutter's smooth clip, the
camera's steps scaled by a drawn `walk` so that up to fourteen neighbours still see the frame, two neighbours brighter and darker.

Placement: every caller plane of a primitive lies at a drawn byte offset inside its buffer -- images, masks and the other byte planes at one of
PLANE_OFFSETS, cells, records and counters at one of CELL_OFFSETS: the minimum alignment the headers under include/ admit (4 and 8 bytes), which
no torch allocation ever has.  case.place holds the draws, taken in turn by the driver.

merge's weight 65536 is one past the documented range (include/rsdsfm_retime.h: 0 .. 65535; the definition asserts it): that draw must be
REFUSED with every output untouched, and counts as a trivial case.

REGRESSIONS: (seed, n) of every case that ever failed on the GPU, appended in the commit that fixes the failure;
tests/test_gpu_temporal_fuzz.py::test_regressions runs them on both library builds."""
import types

import numpy as np

import denoise_cases as dcases
import denoise_spec_numpy as denoise_spec
import plate_cases as pcases
import plate_spec_numpy as plate_spec
import retime_cases as rcases
import retime_spec_numpy as retime_spec
import shutter_cases as scases
import shutter_spec_numpy as shutter_spec
import stabilize_blend_spec_numpy as blend_spec
import stage_fuzz_cases as G
import superres_cases as ucases
import superres_spec_numpy as superres_spec
from stage_fuzz_cases import BIASED, MAX_PIXELS, _data_rng, _data_seed, _dense_params, _pick, _size

REGRESSIONS = []

PRIMITIVES = ("merge", "shutter", "sums", "denoise", "superres_render", "superres_accumulate", "plate")
FRAMES = ("retime_frame", "shutter_frame", "denoise_frame", "superres_frame", "plate_frame")
FAMILIES = PRIMITIVES + FRAMES
TILE = ("denoise", "superres_accumulate", "plate")
CHAINS = ("shutter", "denoise", "superres_accumulate")
SIZED_AS = {f: "seam" for f in TILE}  # stage_fuzz_cases.STRIP_SHARE / STRIP_WIDE: a strip in 0.2 of the draws, 0.7 of them wide
STAGE_SHARE = 0.25
PLANE_OFFSETS, CELL_OFFSETS = (0, 4, 8, 12), (0, 8)
FRAME_ROWS, FRAME_COLS = 70, 140
FRAME_WORK = 150000  # nsrc * scale^2 * rows * cols of a frame call: the definitions render every source in numpy
WEIGHTS = [0, 1, 32768, 32769, 65535, 65536, None]
WEIGHT_REFUSED = 65536
RECORD_KEYS = [None, "plain", "low", "high", "small", "zero"]


def _chain_params(rng, rows, cols):
    """the draws of the denoise's chain, shared by the super-resolution's accumulate"""
    L = int(_pick(rng, [0, 1, 2, int(rng.integers(3, 15))], p=[0.1, 0.2, 0.2, 0.5]))  # first and last together, apart, and with mid steps between
    records = None if rng.random() < 0.25 else tuple(_pick(rng, RECORD_KEYS) for _ in range(L))
    return dict(L=L, records=records, gain_mode=int(rng.random() < 0.3), min_overlap=int(_pick(rng, [0, 1, 64, rows * cols + 1])),
                strength=int(_pick(rng, [1, 12, 255, int(rng.integers(1, 256))])), with_weight=bool(rng.random() < 0.7), with_counts=bool(rng.random() < 0.7))


def _frame_size(rng, work):
    """sides within 70 x 140, half of them from the biased list, rows * cols * work <= FRAME_WORK"""
    while True:
        rows = int(_pick(rng, [b for b in BIASED if b <= FRAME_ROWS])) if rng.random() < 0.5 else int(rng.integers(2, FRAME_ROWS + 1))
        cols = int(_pick(rng, [b for b in BIASED if b <= FRAME_COLS])) if rng.random() < 0.5 else int(rng.integers(2, FRAME_COLS + 1))
        if rows * cols * work <= FRAME_WORK:
            return rows, cols


def _occlusion(rng):
    occlusion = int(rng.integers(0, 2))
    return dict(occlusion=occlusion, search=occlusion * int(rng.integers(0, 2)))


def _neighbours(rng):
    """nsrc 1 .. 15 as a clip of nsrc sources seen from a frame q that has every other one within radius 7; walk: the factor on the builder's
    camera steps (at 1 a source seven frames away has left a frame of these sizes altogether)"""
    nsrc = int(rng.integers(1, 16))
    return dict(nsrc=nsrc, q=int(rng.integers(max(0, nsrc - 8), min(7, nsrc - 1) + 1)), walk=float(_pick(rng, [1.0, 0.3, 0.1], p=[0.3, 0.4, 0.3])))


def random_case(n, seed):
    """-> the record of case n of campaign seed: family, op, rows, cols, strip, channels, params (a dict of Python scalars and tuples), place (the
    placement draws) and, for family "stage", stage: the existing campaign's record"""
    rng = np.random.default_rng([int(seed), int(n), 1000])
    place = dict(planes=tuple(int(_pick(rng, PLANE_OFFSETS)) for _ in range(16)), cells=tuple(int(_pick(rng, CELL_OFFSETS)) for _ in range(4)))
    if rng.random() < STAGE_SHARE:
        st = G.random_case(n, seed)
        return types.SimpleNamespace(seed=int(seed), n=int(n), family="stage", op=st.family, rows=st.rows, cols=st.cols, strip=st.strip, channels=st.channels, params={},
                                     place=place, stage=st)
    family = FAMILIES[int(rng.integers(0, len(FAMILIES)))]
    channels = int(_pick(rng, [1, 3]))
    strip = False
    if family in PRIMITIVES:
        (rows, cols), strip = _size(rng, SIZED_AS.get(family, family))
    if family == "merge":
        b = bool(rng.random() < 0.8)
        weight = _pick(rng, WEIGHTS, p=[0.1, 0.1, 0.15, 0.15, 0.1, 0.05, 0.35])
        p = dict(b=b, weight=(int(rng.integers(0, 65536)) if weight is None else weight) if b else 0, threshold=int(_pick(rng, [0, 8, 24, 255, int(rng.integers(0, 256))])),
                 masks=tuple(_pick(rng, ["pattern", "empty", "full", "random"], p=[0.55, 0.1, 0.1, 0.25]) for _ in range(2)), density=round(G._u(rng, 0.02, 0.98), 3),
                 with_source=bool(rng.random() < 0.7), with_counts=bool(rng.random() < 0.7))
    elif family == "shutter":
        S = int(_pick(rng, [1, 2, 3, 8, 64, int(rng.integers(1, 65))], p=[0.2, 0.2, 0.2, 0.15, 0.05, 0.2]))
        p = dict(S=S, min_samples=int(rng.integers(1, S + 1)), empty=tuple(bool(rng.random() < 0.1) for _ in range(S)), with_coverage=bool(rng.random() < 0.7),
                 with_counts=bool(rng.random() < 0.7))
    elif family == "sums":
        p = dict(mask=_pick(rng, ["pattern", "empty", "full"], p=[0.8, 0.1, 0.1]))
    elif family in ("denoise", "superres_accumulate"):
        p = _chain_params(rng, rows, cols)
    elif family == "superres_render":
        scale = int(_pick(rng, [s for s in (1, 2, 3, 4) if s * s * rows * cols <= MAX_PIXELS]))
        d = _dense_params(rng, rows, cols)
        h, w = int(rng.integers(1, rows + 1)), int(rng.integers(1, cols + 1))
        window = None if rng.random() < 0.5 else (int(rng.integers(0, rows - h + 1)), int(rng.integers(0, cols - w + 1)), h, w)
        p = dict(scale=scale, window=window, mode=d["mode"], q5_mode=d["q5_mode"], iterations=d["iterations"], kind=_pick(rng, ["identity", "pose", "empty"], p=[0.2, 0.72, 0.08]),
                 with_valid=bool(rng.random() < 0.7))
    elif family == "plate":
        L = int(rng.integers(0, 15))
        p = dict(L=L, records=bool(rng.random() < 0.7), phase=int(rng.integers(0, 5)), min_overlap=int(_pick(rng, [0, 1, 1024, 6000])), gain_mode=int(rng.random() < 0.2),
                 threshold=int(_pick(rng, [1, 24, 255, int(rng.integers(1, 256))], p=[0.1, 0.3, 0.1, 0.5])),
                 min_votes=int(_pick(rng, [1, 2, 3, int(rng.integers(1, 16))], p=[0.2, 0.2, 0.2, 0.4])), with_votes=bool(rng.random() < 0.7),
                 with_moving=bool(rng.random() < 0.7), with_counts=bool(rng.random() < 0.7))
    elif family == "retime_frame":
        nsrc = int(rng.integers(1, 3))
        rows, cols = _frame_size(rng, nsrc)
        p = dict(nsrc=nsrc, weight=int(rng.integers(1, 65536)), threshold=int(_pick(rng, [0, 8, 24, 255])), iterations=int(rng.integers(0, 4)), **_occlusion(rng),
                 with_source=bool(rng.random() < 0.7), with_counts=bool(rng.random() < 0.7))
    elif family == "shutter_frame":
        nsources, samples = int(rng.integers(2, 4)), int(_pick(rng, [1, 2, 3, 4, 5]))
        rows, cols = _frame_size(rng, 2 * samples)
        p = dict(nsources=nsources, samples=samples, min_samples=int(rng.integers(1, samples + 1)), t=round(G._u(rng, 0.0, nsources - 1.0), 3),
                 shutter=_pick(rng, [0.0, 0.5, round(G._u(rng, 0.0, nsources - 1.0), 3)]), **_occlusion(rng), with_coverage=bool(rng.random() < 0.7),
                 with_counts=bool(rng.random() < 0.7))
    else:
        p = _neighbours(rng)
        scale = int(rng.integers(1, 5)) if family == "superres_frame" else 1
        rows, cols = _frame_size(rng, p["nsrc"] * scale * scale)
        p.update(strength=int(_pick(rng, [1, 12, 255, int(rng.integers(8, 256))], p=[0.05, 0.3, 0.25, 0.4])), gain_mode=int(rng.random() < 0.3), min_overlap=int(_pick(rng, [1, 64, 1024, rows * cols + 1])),
                 iterations=int(rng.integers(0, 4)), with_weight=bool(rng.random() < 0.7), with_counts=bool(rng.random() < 0.7))
        if family == "superres_frame":
            p.update(scale=scale, occlusion=0, search=0)
        else:
            p.update(_occlusion(rng))
        if family == "plate_frame":
            p.update(min_votes=int(_pick(rng, [1, 2, 3, int(rng.integers(1, 16))], p=[0.2, 0.2, 0.2, 0.4])), with_moving=bool(rng.random() < 0.7))
    return types.SimpleNamespace(seed=int(seed), n=int(n), family=family, op=family, rows=rows, cols=cols, strip=strip, channels=channels, params=p, place=place)


def describe(case):
    if case.family == "stage":
        return "stage: " + G.describe(case.stage)
    return "%s %dx%d x%d params %r place %r" % (case.family, case.rows, case.cols, case.channels, case.params, case.place)


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def _salt(case):
    return case.n % 1000 + 7 * case.seed


def _mask_of(kind, pattern, density, rng):
    if kind == "empty":
        return np.zeros_like(pattern)
    if kind == "full":
        return np.maximum(pattern, 1)
    if kind == "random":
        return ((rng.random(pattern.shape) < density) * rng.choice(np.array([1, 1, 2, 77, 128, 255]), size=pattern.shape)).astype(np.uint8)
    return pattern


def _records(p, channels):
    if p["records"] is None or p["L"] == 0:
        return None
    rec = dcases.records(channels)
    return [None if k is None else rec[k] for k in p["records"]]


def _clip(case):
    """the shutter's smooth clip of nsrc sources under the case's draws, as a denoise case (frame q, every other source within the radius)"""
    p = case.params
    clip = scases.smooth_clip(case.rows, case.cols, case.channels, _data_seed(case) % 100000, t=0.0, shutter=0.0, samples=1, nsources=p["nsrc"])
    clip = dict(clip, c=clip["c"] * p["walk"], c_path=clip["c_path"] * p["walk"])
    if p["nsrc"] >= 3:  # a brighter and a darker neighbour, as denoise_cases.gained_clip: the record gives a gain other than 1
        fr = clip["frames"]
        clip = dict(clip, frames=[fr[0], np.clip(fr[1].astype(np.int64) * 5 // 4, 0, 255).astype(np.uint8), np.clip(fr[2].astype(np.int64) * 4 // 5, 0, 255).astype(np.uint8)] + fr[3:])
    return dcases.from_shutter(clip, "fuzz", p["q"], radius=7, strength=p["strength"], min_overlap=p["min_overlap"], gain_mode=p["gain_mode"], occlusion=p["occlusion"],
                               search=p["search"], iterations=p["iterations"])


def inputs(case, pose_table):
    """-> the case's arrays (a dict; the frame calls': the builders' case dict under "case")"""
    rows, cols, ch, p = case.rows, case.cols, case.channels, case.params
    if case.family == "stage":
        return G.inputs(case.stage, pose_table)
    rng = _data_rng(case, 50)
    if case.family == "merge":
        ia, ma, ib, mb = rcases.merge_layers(rows, cols, ch, _salt(case))
        ma, mb = _mask_of(p["masks"][0], ma, p["density"], rng), _mask_of(p["masks"][1], mb, p["density"], rng)
        return dict(ia=ia, ma=ma, ib=ib if p["b"] else None, mb=mb if p["b"] else None)
    if case.family == "shutter":
        ss = scases.samples(rows, cols, ch, p["S"], _salt(case))
        return dict(samples=[(i, np.zeros_like(m) if e else m) for (i, m), e in zip(ss, p["empty"])])
    if case.family == "sums":
        ref, rmask = dcases.reference(rows, cols, ch, _salt(case))
        (layer, lmask), = dcases.layers(ref, rows, cols, ch, 1, _salt(case))
        lmask = _mask_of(p["mask"], lmask, 0.0, rng)
        source = np.where(rmask != 0, rng.choice(np.array([1, 1, 1, 2, 5]), size=(rows, cols)), 0).astype(np.uint8)
        return dict(image=ref, source=source, layer=layer, lmask=lmask)
    if case.family == "denoise":
        ref, rmask = dcases.reference(rows, cols, ch, _salt(case))
        return dict(ref=ref, rmask=rmask, layers=dcases.layers(ref, rows, cols, ch, p["L"], _salt(case)), records=_records(p, ch))
    if case.family == "superres_accumulate":
        ref, near, prox = ucases.reference(rows, cols, ch, _salt(case))
        return dict(ref=ref, near=near, prox=prox, layers=ucases.layers(ref, rows, cols, ch, p["L"], _salt(case)), records=_records(p, ch))
    if case.family == "superres_render":
        return ucases.render_source(rows, cols, ch, p["kind"], _salt(case))
    if case.family == "plate":
        ref, rmask, layers = pcases.median_inputs((rows, cols), ch, p["L"], _salt(case))
        return dict(ref=ref, rmask=rmask, layers=layers, records=pcases.layer_records(ch, p["L"], p["phase"]) if p["records"] and p["L"] else None)
    if case.family == "retime_frame":
        c = rcases.smooth_pair(rows, cols, ch, _data_seed(case) % 100000, p["weight"], p["threshold"], p["occlusion"], p["search"], "fuzz", p["iterations"])
        return dict(case=c if p["nsrc"] == 2 else rcases.one_source(c, "fuzz"))
    if case.family == "shutter_frame":
        return dict(case=scases.smooth_clip(rows, cols, ch, _data_seed(case) % 100000, p["t"], p["shutter"], p["samples"], p["min_samples"], p["nsources"], "fuzz",
                                            occlusion=p["occlusion"], search=p["search"]))
    c = _clip(case)
    if case.family == "superres_frame":
        c = ucases._with_scale(c, p["scale"])
    if case.family == "plate_frame":
        c = dict(c, threshold=p["strength"], min_votes=p["min_votes"])
    return dict(case=c)


# ---------------------------------------------------------------------------------------------------
# the definitions' outputs
# ---------------------------------------------------------------------------------------------------
def _chain_kw(p):
    return dict(min_overlap=p["min_overlap"] or blend_spec.MIN_OVERLAP_DEFAULT, gain_mode=p["gain_mode"], strength=p["strength"])


def expected(case, inp):
    """-> the definition's outputs; the chains' with cells_before, the cells as the last step must find and leave them (None: the preset)"""
    p = case.params
    if case.family == "stage":
        return G.expected(case.stage, inp)
    if case.family == "merge":
        if p["weight"] == WEIGHT_REFUSED:
            return dict(refused=True)
        return retime_spec.merge(inp["ia"], inp["ma"], inp["ib"], inp["mb"], p["weight"], p["threshold"])
    if case.family == "shutter":
        cells, before = None, None
        for j, (image, mask) in enumerate(inp["samples"]):
            before = cells
            cells = shutter_spec.accumulate(cells, image, mask, j == 0)
        return dict(shutter_spec.resolve(cells, p["S"], p["min_samples"], case.channels == 1), cells_before=before)
    if case.family == "sums":
        return dict(sums=blend_spec.overlap_sums(inp["image"], inp["source"], inp["layer"], inp["lmask"]))
    if case.family == "denoise":
        r = denoise_spec.denoise(inp["ref"], inp["rmask"], inp["layers"], inp["records"], **_chain_kw(p))
        return dict(r, cells_before=r["cells"][-2] if p["L"] >= 2 else None)
    if case.family == "superres_accumulate":
        r = superres_spec.accumulate(inp["ref"], inp["near"], inp["prox"], inp["layers"], inp["records"], **_chain_kw(p))
        return dict(r, cells_before=r["cells"][-2] if p["L"] >= 2 else None)
    if case.family == "superres_render":
        return superres_spec.render(inp["image"], inp["depth"], inp["R"], inp["t"], inp["K"], inp["M"], inp["m"], p["scale"], p["window"], p["mode"], p["q5_mode"], p["iterations"])
    if case.family == "plate":
        return plate_spec.median(inp["ref"], inp["rmask"], inp["layers"], None if inp["records"] is None else list(inp["records"]),
                                 p["min_overlap"] or plate_spec.MIN_OVERLAP_DEFAULT, p["gain_mode"], p["threshold"], p["min_votes"])
    run = dict(retime_frame=rcases.run_spec, shutter_frame=scases.run_spec, denoise_frame=dcases.run_spec, superres_frame=ucases.run_spec, plate_frame=pcases.run_spec)
    return run[case.family](inp["case"])


def _binary(m):
    return set(np.unique(m).tolist()) <= {0, 1}


def undefined(case, inp, want):
    """-> the reasons (strings) why the definition's output for this case is not one a kernel can be held to; empty for a good case"""
    if case.family == "stage":
        return G.undefined(case.stage, inp, want)
    if want.get("refused"):
        return []
    pixels = case.rows * case.cols * (case.params.get("scale", 1) ** 2 if case.family in ("superres_render", "superres_frame") else 1)
    bad = []
    if case.family == "sums":
        if int(want["sums"][0]) > pixels or want["sums"][1 + 2 * case.channels:].any():
            bad.append("sums: the count or the unused words")
    elif case.family == "superres_render":
        if want["prox"].max(initial=0) > superres_spec.PROX_MAX or want["bil"][want["prox"] == 0].any() or want["near"][want["prox"] == 0].any():
            bad.append("render: proximity, or bytes where it is 0")
    else:
        if not _binary(want["mask"]) or sum(want["counts"]) != pixels or want["image"][want["mask"] == 0].any():
            bad.append("%s: mask, counts or image" % case.family)
        if case.family in ("plate", "plate_frame") and (want["votes"].max(initial=0) > 15 or want["moving"].max(initial=0) > 3):
            bad.append("plate: votes or flag")
    return bad


def trivial(case, inp, want):
    """-> {what: bool} for every call the case makes: whether the definition's own output is one that a kernel doing nothing would also give --
    a merge with no set pixel (or a refused one), a chain that averages nothing, a plate with no votes, a render with an empty proximity plane"""
    if case.family == "stage":
        return G.trivial(case.stage, inp, want)
    f = case.family
    if f in ("merge", "retime_frame"):
        return {f: bool(want.get("refused")) or want["counts"][0] == case.rows * case.cols}
    if f in ("shutter", "shutter_frame"):
        return {f: not want["mask"].any()}
    if f == "sums":
        return {f: int(want["sums"][0]) == 0}
    if f == "superres_render":
        return {f: not want["prox"].any()}
    if f in ("plate", "plate_frame"):
        return {f: not want["votes"].any()}
    return {f: want["counts"][2] == 0}
