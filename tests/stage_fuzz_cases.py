"""The generator of the post-solve stages' randomised campaign (tests/fuzz_stages.py on the GPU, tests/test_stage_fuzz_cpu.py here): case n
of campaign `seed` is random_case(n, seed), a record of plain Python values that depends on nothing but (n, seed); inputs(case, pose_table)
builds its arrays with the builders of the families' own tests/*_cases.py modules, expected(case, inp) runs the family's definition
(tests/*_spec_numpy.py), undefined(case, inp, want) names the spec outputs that are not well defined (a failure of the generator, never a
skip) and trivial(case, inp, want) says whether the spec's own output is one a wrong kernel could also give (nothing linked, filled, kept or written).

Families (drawn, not dealt in turn): flow_check, link, fuse, dense, stabilize, fill, crop (the window search, then one frame through a
window), seam (the distance, then -- op "blend" -- one layer) and inpaint.  Sides in [2, 300], half of the draws from BIASED; a strip has one
side from STRIP_LONG and the other in [2, 8], wide or tall.  One case in about ten is a strip: the families whose kernels have an edge at
1024 columns of ONE row (crop: the row scan's carry; seam: the distance's row segments) draw one more often (STRIP_SHARE).
rows * cols <= 90000 keeps the numpy specs fast.

REGRESSIONS: (seed, n) of every case that ever failed on the GPU, appended in the commit that fixes the failure;
tests/test_gpu_stage_fuzz.py::test_regressions runs them on both library builds."""
import types

import numpy as np

import flow_check_cases
import flow_check_spec_numpy as flow_check_spec
import fuse_cases
import fuse_spec_numpy as fuse_spec
import link_cases
import link_spec_numpy as link_spec
import rectify_dense_cases as dense_cases
import rectify_dense_spec_numpy as dense_spec
import stabilize_blend_cases as blend_cases
import stabilize_blend_spec_numpy as blend_spec
import stabilize_cases as stab_cases
import stabilize_crop_cases as crop_cases
import stabilize_crop_spec_numpy as crop_spec
import stabilize_fill_spec_numpy as fill_spec
import stabilize_inpaint_cases as inpaint_cases
import stabilize_inpaint_spec_numpy as inpaint_spec
import stabilize_spec_numpy as stab_spec

REGRESSIONS = []

FAMILIES = ("flow_check", "link", "fuse", "dense", "stabilize", "fill", "crop", "seam", "inpaint")
WITH_CHANNELS = ("dense", "stabilize", "fill", "crop", "seam", "inpaint")
BIASED = [2, 3, 4, 5] + list(range(15, 19)) + list(range(31, 35)) + list(range(63, 67)) + list(range(127, 131))
STRIP_LONG = [1023, 1024, 1025, 1026, 1100, 2047, 2048, 2049, 2050]
STRIP_SHARE = dict(crop=0.4, seam=0.2)  # every other family: 0.09; (0.4 + 0.2 + 7 * 0.09) / 9 = 0.137 of all cases
STRIP_WIDE = dict(crop=0.75, seam=0.7)   # the share of strips that are wide (every other family: 0.5): those edges lie along a row
MAX_PIXELS = 90000
FEATHERS = [1, 2, 8, 16, 63, 64]
M_N_AXIS, m_N = np.array([-0.03, 0.04, -0.02]), np.array([-0.1, 0.05, -0.15])  # the fill tests' neighbour pose
M_STD_AXIS = np.array([0.01, -0.015, 0.02])  # stabilize_cases.M_STD's rotation vector


def _pick(rng, values, p=None):
    return values[int(rng.choice(len(values), p=p))]


def _side(rng):
    return int(_pick(rng, BIASED)) if rng.random() < 0.5 else int(rng.integers(2, 301))


def _size(rng, family):
    if rng.random() < STRIP_SHARE.get(family, 0.09):
        long_side, short_side = int(_pick(rng, STRIP_LONG)), int(rng.integers(2, 9))
        return ((short_side, long_side) if rng.random() < STRIP_WIDE.get(family, 0.5) else (long_side, short_side)), True
    while True:
        rows, cols = _side(rng), _side(rng)
        if rows * cols <= MAX_PIXELS:
            return (rows, cols), False


def _u(rng, lo, hi):
    return float(rng.uniform(lo, hi))


def _holes(rng):
    return _pick(rng, [0.0, 0.3, 0.97, round(_u(rng, 0.05, 0.9), 3)], p=[0.05, 0.3, 0.15, 0.5])


def _dense_params(rng, rows, cols):
    """the dense rectifier's draws, shared by every family that renders a frame"""
    p = dict(mode=int(rng.integers(0, 2)), q5_mode=int(rng.integers(0, 2)), iterations=int(_pick(rng, [0, 1, 2, 3, 4, 5, 6], p=[0.4] + [0.1] * 6)),
             holes=_pick(rng, [0.0, 0.4, 0.7, round(_u(rng, 0.05, 0.95), 3)], p=[0.1, 0.4, 0.2, 0.3]), specials=bool(rng.random() < 0.2),
             none_valid=bool(rng.random() < 0.04), roll=(int(rng.integers(0, rows)), int(rng.integers(0, cols))),
             motion=_pick(rng, [1.0, round(_u(rng, 0.0, 2.0), 3)]), block=None, corner=None)
    if rows >= 8 and cols >= 8 and rng.random() < 0.3:
        h, w = int(rng.integers(1, rows // 2)), int(rng.integers(1, cols // 2))
        p["block"] = (int(rng.integers(0, rows - h)), int(rng.integers(0, cols - w)), h, w)
    if rows >= 8 and cols >= 8 and rng.random() < 0.2:
        p["corner"] = (int(rng.integers(1, rows // 2)), int(rng.integers(1, cols // 2)))
    return p


def _pose_params(rng):
    """a virtual pose between the identity and several times the standard one, about the stabiliser's or the fill's axis"""
    return dict(pose_axis=_pick(rng, ["std", "neighbour"]), pose_scale=_pick(rng, [0.0, 1.0, round(_u(rng, 0.0, 4.0), 3)], p=[0.1, 0.3, 0.6]))


def _inout_params(rng, rows, cols):
    return dict(start=_pick(rng, ["empty", "full", "bands", "random"], p=[0.2, 0.05, 0.4, 0.35]), sid=int(rng.integers(2, 256)),
                with_source=bool(rng.random() < 0.7), with_count=bool(rng.random() < 0.7))


def _window_params(rng, rows, cols):
    kind = _pick(rng, ["full", "random", "one", "found"], p=[0.25, 0.35, 0.15, 0.25])
    h, w = int(rng.integers(1, rows + 1)), int(rng.integers(1, cols + 1))
    return dict(window_kind=kind, window=dict(full=(0, 0, rows, cols), one=(int(rng.integers(0, rows)), int(rng.integers(0, cols)), 1, 1),
                                              random=(int(rng.integers(0, rows - h + 1)), int(rng.integers(0, cols - w + 1)), h, w), found=None)[kind])


def random_case(n, seed):
    """-> the record of case n of campaign seed: family, op, rows, cols, strip, channels, params (a dict of Python scalars and tuples)"""
    rng = np.random.default_rng([int(seed), int(n)])
    family = FAMILIES[int(rng.integers(0, len(FAMILIES)))]
    (rows, cols), strip = _size(rng, family)
    channels = int(_pick(rng, [1, 3])) if family in WITH_CHANNELS else 0
    op = family
    if family == "flow_check":
        p = dict(a1=_pick(rng, [None, 0.0, round(_u(rng, 0.0, 0.1), 4)]), a2=_pick(rng, [None, 0.0, 20.0, round(_u(rng, 0.0, 2.0), 3)]), specials=bool(rng.random() < 0.7),
                 extra=int(rng.integers(0, 9)), in_place=bool(rng.random() < 0.3), without=tuple(k for k in ("masked", "resid", "count") if rng.random() < 0.2))
        if rng.random() < 0.1:
            p["a1"], p["a2"] = 0.0, 0.0
    elif family == "link":
        links = int(rng.integers(1, 6))
        kinds = ["base", "special", "planted", "wide", "two_values", "negative", "empty"]
        p = dict(links=links, kinds=tuple(_pick(rng, kinds, p=[0.4, 0.15, 0.1, 0.15, 0.1, 0.05, 0.05]) for _ in range(links)), holes=tuple(_holes(rng) for _ in range(links)),
                 radix_bits=_pick(rng, [None, 8]), global_shutter=bool(rng.random() < 0.3), tol=_pick(rng, [None, 0.0, 0.05, round(_u(rng, 0.0, 0.5), 3)]),
                 min_links=_pick(rng, [None, 0, 1, 100, rows * cols]), own_planes=bool(rng.random() < 0.6))
    elif family == "fuse":
        pairs = int(rng.integers(2, 6))
        p = dict(pairs=pairs, holes=_holes(rng), broken=tuple(_pick(rng, [None, "invalid", "nan", "negative"], p=[0.8, 0.08, 0.06, 0.06]) for _ in range(pairs - 1)),
                 tol=_pick(rng, [None, 0.01, round(_u(rng, 0.0, 0.5), 3)]), global_shutter=bool(rng.random() < 0.3), last_field=bool(rng.random() < 0.5),
                 flags=bool(rng.random() < 0.8), planes=bool(rng.random() < 0.6), specials=bool(rng.random() < 0.3))
    elif family == "dense":
        p = dict(_dense_params(rng, rows, cols), without=tuple(k for k in ("mask", "filled", "disp") if rng.random() < 0.25))
    elif family == "stabilize":
        p = dict(_dense_params(rng, rows, cols), **_pose_params(rng), with_valid=bool(rng.random() < 0.6))
    elif family == "fill":
        p = dict(_dense_params(rng, rows, cols), **_pose_params(rng), **_inout_params(rng, rows, cols))
    elif family == "crop":
        planes = int(rng.integers(1, 6))
        empty = 0.0 if rng.random() < 0.15 else float(np.exp(_u(rng, np.log(1e-4), np.log(0.1))))
        p = dict(_dense_params(rng, rows, cols), **_pose_params(rng), **_inout_params(rng, rows, cols), **_window_params(rng, rows, cols), planes=planes,
                 set_value=int(_pick(rng, [1, 255])), empty=round(empty, 6), margin=_pick(rng, [0, 1, 3, None]),
                 max_empty=int(_pick(rng, [0, int(rng.integers(1, 9)), rows * cols], p=[0.5, 0.35, 0.15])))
    elif family == "seam":
        op = "blend" if rng.random() < 0.8 else "distance"
        p = dict(feather=int(_pick(rng, FEATHERS)), mask_kind=int(rng.integers(0, 6)), sparse=bool(rng.random() < 0.3), sid=int(rng.integers(2, 256)),
                 min_overlap=int(_pick(rng, [0, 1, 64, rows * cols + 1], p=[0.2, 0.4, 0.3, 0.1])), gain=bool(rng.random() < 0.75), with_counts=bool(rng.random() < 0.7))
    else:
        p = dict(mask_kind=_pick(rng, ["set", "empty", "last", "bands", "random-255", "rectangle"], p=[0.05, 0.05, 0.15, 0.25, 0.25, 0.25]),
                 with_source=bool(rng.random() < 0.7), with_count=bool(rng.random() < 0.7))
        h, w = int(rng.integers(1, rows + 1)), int(rng.integers(1, cols + 1))
        p["rectangle"] = (int(rng.integers(0, rows - h + 1)), int(rng.integers(0, cols - w + 1)), h, w)
    return types.SimpleNamespace(seed=int(seed), n=int(n), family=family, op=op, rows=rows, cols=cols, strip=strip, channels=channels, params=p)


def describe(case):
    return "%s/%s %dx%d x%d params %r" % (case.family, case.op, case.rows, case.cols, case.channels, case.params)


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def _data_rng(case, salt=0):
    return np.random.default_rng([case.seed, case.n, 1 + salt])


def _data_seed(case):
    return (case.seed * 1000003 + case.n) % (1 << 31)


def _flow_check_inputs(case):
    rows, cols, p = case.rows, case.cols, case.params
    fwd, bwd, _ = flow_check_cases.fields(rows, cols, specials=p["specials"])
    rng = _data_rng(case)
    for _ in range(p["extra"]):  # NaN / inf vectors and landing points exactly on the last column and row, at drawn pixels
        i, j, what = int(rng.integers(0, rows)), int(rng.integers(0, cols)), int(rng.integers(0, 5))
        fwd[i, j] = [(np.nan, 0.5), (0.25, np.inf), (float(cols - 1 - j), 0.0), (0.0, float(rows - 1 - i)), (float(cols - 1 - j), float(rows - 1 - i))][what]
    return dict(fwd=fwd, bwd=bwd)


def _link_one(kind, rows, cols, holes, salt):
    if kind == "base":
        return link_cases.base_case(rows, cols, holes, salt=salt)
    if kind == "special":
        return link_cases.special_case(rows, cols)[0]
    if kind == "planted":
        return link_cases.planted_case(rows, cols, [0.8125, 1.25, 3.0], share=max(1.0 - holes, 0.05), salt=17 + salt)
    if kind == "wide":
        return link_cases.wide_ratios(rows, cols, salt=19 + salt)
    if kind == "two_values":
        return link_cases.two_values_on_the_boundary(rows, cols)
    if kind == "negative":
        return link_cases.negative_prediction_case(rows, cols)
    return link_cases.empty_case(rows, cols)


def _link_inputs(case):
    """links + 1 maps: link q is its kind's field and motion from map q to map q + 1; map 0 is link 0's Z_p and map q + 1 link q's Z_n, so a
    single link is its kind exactly and a longer chain mixes them"""
    rows, cols, p = case.rows, case.cols, case.params
    parts = [_link_one(kind, rows, cols, h, 31 + 7 * q + case.n % 1000) for q, (kind, h) in enumerate(zip(p["kinds"], p["holes"]))]
    maps = [parts[0]["Zp"]] + [d["Zn"] for d in parts]
    return dict(fields=[d["F"] for d in parts], maps=maps, vs=[d["v"] for d in parts] + [np.zeros(3)], ws=[d["w"] for d in parts] + [np.zeros(3)],
                ks=[float(d["k"]) for d in parts] + [0.0], K=link_cases.camera(rows, cols), gamma=link_cases.GAMMA)


def _fuse_inputs(case):
    rows, cols, p = case.rows, case.cols, case.params
    ch = fuse_cases.chain_case(rows, cols, p["pairs"], p["holes"], salt=case.n % 1000)
    for l, kind in enumerate(p["broken"]):
        if kind:
            ch["records"][l] = dict(ch["records"][l], **fuse_cases.BROKEN[kind])
    if p["specials"]:
        rng = _data_rng(case)
        for q in range(p["pairs"]):
            for value in (np.nan, np.inf, -np.inf, -1.5):
                ch["maps"][q][int(rng.integers(0, rows)), int(rng.integers(0, cols))] = value
        for q in range(p["pairs"]):
            for value in ((np.nan, 1.0), (1.0, -np.inf), (0.0, 0.0), (-0.0, 0.0), (1e300, 0.0)):
                ch["fields"][q][int(rng.integers(0, rows)), int(rng.integers(0, cols))] = value
    if not p["last_field"]:
        ch["fields"] = ch["fields"][:-1]
    return ch


def _rendered(case, pose_table, neighbour=False):
    """the dense rectifier's inputs at this size (tests/rectify_dense_cases.py), rolled by the case's offsets, under the case's motion"""
    rows, cols, p = case.rows, case.cols, case.params
    K, image, depth = dense_cases.inputs(rows, cols, channels=case.channels, holes=p["holes"], block=p["block"], corner=p["corner"], specials=p["specials"],
                                         none_valid=p["none_valid"])
    image, depth = np.ascontiguousarray(np.roll(image, p["roll"], axis=(0, 1))), np.ascontiguousarray(np.roll(depth, p["roll"], axis=(0, 1)))
    if neighbour:
        image = np.ascontiguousarray(image[::-1])
    R, t = pose_table(dense_cases.POSE["v"] * p["motion"], dense_cases.POSE["w"] * p["motion"], dense_cases.POSE["k"], dense_cases.POSE["gamma"], rows)
    return dict(K=K, image=image, depth=depth, R=np.ascontiguousarray(R).reshape(rows, 9), t=np.ascontiguousarray(t))


def _pose(case):
    p = case.params
    if p["pose_axis"] == "std":
        return link_spec.rodrigues(p["pose_scale"] * M_STD_AXIS), p["pose_scale"] * stab_cases.m_STD
    return link_spec.rodrigues(p["pose_scale"] * M_N_AXIS), p["pose_scale"] * m_N


def _inout_planes(case, rng):
    rows, cols, p = case.rows, case.cols, case.params
    if p["start"] in ("empty", "full"):
        mask = np.full((rows, cols), int(p["start"] == "full"), dtype=np.uint8)
    elif p["start"] == "bands":
        mask = inpaint_cases.masks(rows, cols, _data_seed(case))[3][1].copy()
    else:
        mask = (rng.random((rows, cols)) < 0.5).astype(np.uint8)
    image = inpaint_cases.image_of(rows, cols, case.channels, _data_seed(case) + 1)
    source = (mask * rng.choice(np.array([1, 2, 3], dtype=np.uint8), size=(rows, cols))).astype(np.uint8)
    return dict(image=image, mask=mask, source=source)


def inputs(case, pose_table):
    """-> the case's arrays; pose_table: oracle_py.pose_table (the per-scanline poses of a motion)"""
    rows, cols, p = case.rows, case.cols, case.params
    if case.family == "flow_check":
        return _flow_check_inputs(case)
    if case.family == "link":
        return _link_inputs(case)
    if case.family == "fuse":
        return _fuse_inputs(case)
    if case.family == "dense":
        return _rendered(case, pose_table)
    if case.family == "stabilize":
        M, m = _pose(case)
        return dict(_rendered(case, pose_table), M=M, m=m)
    if case.family in ("fill", "crop"):
        M, m = _pose(case)
        rng = _data_rng(case)
        d = dict(_rendered(case, pose_table, neighbour=True), M=M, m=m, start=_inout_planes(case, rng))
        if case.family == "crop":
            d["masks"] = list(crop_cases.random_masks(rows, cols, p["planes"], p["empty"] / p["planes"], _data_seed(case), set_value=p["set_value"]))
        return d
    if case.family == "seam":
        if case.op == "distance":
            return dict(mask=blend_cases.distance_masks(rows, cols, _data_seed(case))[p["mask_kind"]][1])
        e = blend_cases.layer_case(rows, cols, case.channels, _data_seed(case), p["feather"], sparse=p["sparse"])
        return dict(e, own=(e["dist"] != 0).astype(np.uint8))  # layer_case's dist is the own mask's: set exactly where it is not 0
    image = inpaint_cases.image_of(rows, cols, case.channels, _data_seed(case))
    if p["mask_kind"] == "rectangle":
        mask = np.ones((rows, cols), dtype=np.uint8)
        y0, x0, h, w = p["rectangle"]
        mask[y0:y0 + h, x0:x0 + w] = 0
    else:
        mask = dict(inpaint_cases.masks(rows, cols, _data_seed(case)))[p["mask_kind"]]
    return dict(image=image, mask=mask)


# ---------------------------------------------------------------------------------------------------
# the definitions' outputs
# ---------------------------------------------------------------------------------------------------
def spec_min_overlap(p):
    return p["min_overlap"] or blend_spec.MIN_OVERLAP_DEFAULT


def _dense_kw(p):
    return dict(mode=p["mode"], q5_mode=p["q5_mode"], iterations=p["iterations"])


def expected(case, inp):
    rows, cols, p = case.rows, case.cols, case.params
    if case.family == "flow_check":
        kw = {k: p[k] for k in ("a1", "a2") if p[k] is not None}
        return flow_check_spec.flow_check(inp["fwd"], inp["bwd"], **kw)
    if case.family == "link":
        kw = dict(tol=link_spec.TOL_DEFAULT if p["tol"] is None else p["tol"], min_links=link_spec.MIN_LINKS_DEFAULT if p["min_links"] is None else p["min_links"])
        return dict(links=[link_spec.link(inp["fields"][q], inp["maps"][q], inp["vs"][q], inp["ws"][q], inp["ks"][q], inp["maps"][q + 1], inp["K"], inp["gamma"],
                                          p["global_shutter"], **kw) for q in range(p["links"])])
    if case.family == "fuse":
        return fuse_spec.fuse(inp["fields"], inp["maps"], inp["vs"], inp["ws"], inp["ks"], inp["records"], inp["K"], inp["gamma"], p["global_shutter"],
                              link_spec.TOL_DEFAULT if p["tol"] is None else p["tol"])
    if case.family == "dense":
        return dense_spec.rectify_dense(inp["image"], inp["depth"], inp["R"], inp["t"], *inp["K"], **_dense_kw(p))
    if case.family == "stabilize":
        return stab_spec.stabilize_frame(inp["image"], inp["depth"], inp["R"], inp["t"], inp["K"], inp["M"], inp["m"], **_dense_kw(p))
    if case.family == "fill":
        out = {k: v.copy() for k, v in inp["start"].items()}
        out["count"] = fill_spec.fill_from(out["image"], out["mask"], out["source"], inp["image"], inp["depth"], inp["R"], inp["t"], inp["K"], inp["M"], inp["m"], p["sid"],
                                           **_dense_kw(p))
        return out
    if case.family == "crop":
        found = crop_spec.crop_window(inp["masks"], p["max_empty"], crop_spec.MARGIN_DEFAULT if p["margin"] is None else p["margin"])
        window = p["window"] if p["window_kind"] != "found" else (found if found[2] else (0, 0, rows, cols))
        out = {k: v.copy() for k, v in inp["start"].items()}
        out["count"] = crop_spec.fill_from_window(out["image"], out["mask"], out["source"], inp["image"], inp["depth"], inp["R"], inp["t"], inp["K"], inp["M"], inp["m"],
                                                  p["sid"], window, **_dense_kw(p))
        return dict(out, found=found, window=tuple(int(v) for v in window))
    if case.family == "seam":
        T = p["feather"]
        if case.op == "distance":
            return dict(dist=blend_spec.seam_distance(inp["mask"], T))
        image, mask, source = inp["image"].copy(), inp["mask"].copy(), inp["source"].copy()
        sums = blend_spec.overlap_sums(image, source, inp["layer"], inp["lmask"])
        G = blend_spec.gains(sums, case.channels, spec_min_overlap(p), 0 if p["gain"] else 1)
        counts = blend_spec.blend_layer(image, mask, source, inp["dist"], T, inp["layer"], inp["lmask"], p["sid"], G)
        return dict(dist=blend_spec.seam_distance(inp["own"], T), image=image, mask=mask, source=source, sums=sums, counts=counts, gains=G)
    image, source = inp["image"].copy(), np.zeros((rows, cols), dtype=np.uint8)
    return dict(image=image, source=source, count=inpaint_spec.inpaint(image, inp["mask"], source))


def undefined(case, inp, want):
    """-> the reasons (strings) why the definition's output for this case is not one a kernel can be held to; empty for a good case"""
    rows, cols, p = case.rows, case.cols, case.params
    bad = []
    binary = lambda m: set(np.unique(m).tolist()) <= {0, 1}
    if case.family == "flow_check":
        if not binary(want["mask"]) or np.isnan(want["resid"]).any() or not np.isfinite(want["masked"]).all() or want["count"] != int(want["mask"].sum()):
            bad.append("flow check: mask, residual or masked field")
    elif case.family == "link":
        for q, w in enumerate(want["links"]):
            r = w["plane"][w["plane"] != 0].view(np.float64)
            if not (np.isfinite(r).all() and (r > 0).all()) or w["n"] != r.size or np.isnan(w["ratio"]) != (w["n"] == 0) or not 0 <= w["agree"] <= w["n"]:
                bad.append("link %d: plane or record" % q)
    elif case.family == "fuse":
        for q in range(p["pairs"]):
            f, rec = want["fused"][q], want["records"][q]
            if not (np.isfinite(f).all() and (f >= 0).all()) or (want["flags"][q] >= 32).any() or rec["own"] + rec["filled_prev"] + rec["filled_next"] + rec["left"] != rows * cols:
                bad.append("fuse pair %d: fused map, flags or record" % q)
    elif case.family in ("dense", "stabilize"):
        if np.isnan(want["filled"]).any() or not binary(want["mask"]) or want["image"][want["mask"] == 0].any():
            bad.append("%s: filled map, mask or image" % case.family)
        if case.family == "stabilize" and want["valid"] != int(want["mask"].sum()):
            bad.append("stabilize: valid")
    elif case.family in ("fill", "crop"):
        start = inp["start"]
        taken = (want["mask"] != 0) & (start["mask"] == 0)
        if not binary(want["mask"]) or want["count"] != int(taken.sum()) or not (want["source"][taken] == p["sid"]).all() or not np.array_equal(want["source"][~taken], start["source"][~taken]):
            bad.append("%s: mask, source or count" % case.family)
        if case.family == "crop":
            r0, c0, h, w = want["found"]
            if not (0 <= r0 and 0 <= c0 and r0 + h <= rows and c0 + w <= cols and (h == 0) == (w == 0)):
                bad.append("crop: window %r" % (want["found"],))
    elif case.family == "seam":
        if (want["dist"] > p["feather"]).any():
            bad.append("seam: distance above the feather")
        if case.op == "blend" and (not np.array_equal(want["dist"], inp["dist"]) or min(want["counts"]) < 0 or not all(blend_spec.GAIN_MIN <= g <= blend_spec.GAIN_MAX for g in want["gains"])):
            bad.append("seam: the layer case's distance plane, counts or gains")
    else:
        holes = int((inp["mask"] == 0).sum())
        if want["count"] not in (0, holes) or int((want["source"] == inpaint_spec.SOURCE_INPAINTED).sum()) != want["count"]:
            bad.append("inpaint: count or source")
    return bad


def trivial(case, inp, want):
    """-> {what: bool} for every call the case makes: whether the definition's own output is one that a kernel doing nothing (or everything)
    would also give"""
    if case.family == "flow_check":
        return dict(flow_check=want["count"] in (0, case.rows * case.cols))
    if case.family == "link":
        return dict(link=all(w["n"] == 0 for w in want["links"]))
    if case.family == "fuse":
        return dict(fuse=sum(r["filled_prev"] + r["filled_next"] for r in want["records"]) == 0)
    if case.family == "dense":
        return {}
    if case.family == "stabilize":
        return dict(stabilize=bool((want["mask"] == 0).all() or (want["mask"] == 1).all()))
    if case.family == "fill":
        return dict(fill=want["count"] == 0)
    if case.family == "crop":
        return dict(crop_window=want["found"] == (0, 0, 0, 0), window_frame=want["count"] == 0)
    if case.family == "seam":
        d = dict(seam_distance=not want["dist"].any() or bool((want["dist"] == case.params["feather"]).all()))
        return dict(d, blend=want["counts"] == (0, 0)) if case.op == "blend" else d
    return dict(inpaint=want["count"] == 0)


# ---------------------------------------------------------------------------------------------------
# the window search past one grid (tests/test_gpu_stage_fuzz.py, and at a tenth of the size tests/test_stage_fuzz_cpu.py)
# ---------------------------------------------------------------------------------------------------
def planted_window(side, second=False):
    """on a square frame of `side` (a multiple of 150): a square of side / 25 in the last rows, or -- second -- a larger one in the first"""
    u = side // 150
    return (1 * u, 30 * u, 7 * u, 7 * u) if second else (143 * u, 70 * u, 6 * u, 6 * u)


def planted_mask(side, windows):
    """all empty but the given rectangles: with max_empty = 0 and margin = 0 the window is the largest of them"""
    m = np.zeros((side, side), dtype=np.uint8)
    for r0, c0, h, w in windows:
        m[r0:r0 + h, c0:c0 + w] = 1
    return m
