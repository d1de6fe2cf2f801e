"""Inputs of the sharpness transfer's tests (tests/test_deblur_cpu.py, tests/test_gpu_deblur.py) and of its golden fixture
(tests/golden/make_golden_deblur.py): the denoise's shapes, references, layers, overlap records and impulse positions (tests/denoise_cases.py,
reused as they are), sharpness records that drive every branch of tau, blurred references (so that computed records give tau > 0 too), and
small solved clips for the frame and clip calls: the denoise's shift clip with its own frame blurred or with every frame but its own blurred,
the gained clip and one occlusion clip."""
import numpy as np

import deblur_spec_numpy as spec
import denoise_cases as dcases
import shutter_cases as scases

TILE_ROWS, TILE_COLS = dcases.TILE_ROWS, dcases.TILE_COLS
ACC_SHAPES = dcases.ACC_SHAPES  # (2, 2) .. (70, 300): one word, byte tails, one under, exactly one and one over a tile in each direction
ACC_LAYERS = [1, 2, spec.LAYERS_MAX]
reference, layers, records, impulse_positions = dcases.reference, dcases.layers, dcases.records, dcases.impulse_positions

BLUR = 5  # the clips' box width


def sharp_records():
    """name -> (record [pairs, A_R, A_L, 0], tau at the default margin 4 and min_pairs 1024): tau = 0 by the margin (at it exactly, and below the
    own frame's sharpness, where A_L - A_R would wrap), tau = 0 by min_pairs, taus in 1 .. 31, tau = 31 one below the cap, the cap reached exactly
    and passed, A_R = 0 (the divisor's max(A_R, 1)) with A_L = 0, 1 and 5, and sums near 2^49 (the largest a 16384 x 16384 frame can give)"""
    rec = lambda pairs, ar, al: np.array([pairs, ar, al, 0], dtype=np.uint64)
    return dict(margin=(rec(5000, 1000, 1250), 0), above_margin=(rec(5000, 1000, 1251), 4), equal=(rec(5000, 1000, 1000), 0), duller=(rec(5000, 1000, 3), 0),
                few_pairs=(rec(1023, 100, 1000), 0), enough_pairs=(rec(1024, 100, 1000), 32), half=(rec(5000, 1000, 1500), 8), twice=(rec(5000, 1000, 2000), 16),
                thirty=(rec(5000, 1000, 2937), 30), below_cap=(rec(5000, 1000, 2999), 31), cap=(rec(5000, 1000, 3000), 32), far=(rec(5000, 7, 500000), 32),
                flat_both=(rec(5000, 0, 0), 0), flat_own_1=(rec(5000, 0, 1), 16), flat_own_5=(rec(5000, 0, 5), 32),
                big=(rec(2 ** 29, 2 ** 49 - 3, 2 ** 49 + 2 ** 48), 8), big_cap=(rec(2 ** 29, 2 ** 47, 2 ** 49), 32), big_margin=(rec(2 ** 29, 2 ** 49, 2 ** 49 + 2 ** 47), 0))


def blurred_reference(rows, cols, channels, seed=0, width=BLUR):
    """denoise_cases.reference with its image box-blurred along the rows: layers drawn around the SHARP image are then sharper than it
    -> (blurred image, mask, sharp image)"""
    ref, rmask = reference(rows, cols, channels, seed)
    return spec.box_blur(ref, width), rmask, ref


# ---------------------------------------------------------------------------------------------------
# clips for the frame and the clip call
# ---------------------------------------------------------------------------------------------------
def _with(case, name=None, margin=spec.MARGIN_DEFAULT, min_pairs=spec.MIN_PAIRS_DEFAULT, gate_mode=0, **kw):
    """a denoise case as a deblur case: the three words the denoise does not have; margin is the VALUE (0 .. 64)"""
    out = dict(case, margin=int(margin), min_pairs=int(min_pairs), gate_mode=int(gate_mode), **kw)
    if name:
        out["name"] = name
    return out


def blur_clip(kind, seed=0, channels=3, q=2, radius=2, strength=spec.STRENGTH_DEFAULT, noise=6, width=BLUR, min_pairs=64, name=None, **kw):
    """denoise_cases.shift_clip's scene (five frames of 24 x 40, the texture moved on by 8 columns per frame) with frame q box-blurred over
    `width` columns ("blurred-own") or with every frame BUT q blurred ("sharp-own"); the blur comes before the i.i.d. noise in [-noise, noise].
    min_pairs is small enough for 24 x 40.  The clean SHARP frames ride along as case["clean"]"""
    assert kind in ("blurred-own", "sharp-own")
    clean, f = dcases.shift_clean()
    if channels == 1:
        clean = [np.ascontiguousarray(fr[..., 1]) for fr in clean]
    soft = [spec.box_blur(fr, width) if (n == q) == (kind == "blurred-own") else fr for n, fr in enumerate(clean)]
    rng = np.random.default_rng(9000 + seed)
    frames = [(fr.astype(np.int64) + rng.integers(-noise, noise + 1, size=fr.shape)).astype(np.uint8) for fr in soft]
    case = dcases._clip(name or "%s-%s-%d" % (kind, "bgr" if channels == 3 else "gray", seed), frames, f["depths"], f["Rs"], f["ts"], f["K"], f["A"], f["c"], f["A"],
                        f["c"], f["scales"], q, radius, strength)
    case["clean"] = clean
    return _with(case, min_pairs=min_pairs, **kw)


shift_seen_by_all = dcases.shift_seen_by_all


def all_cases(pose_table):
    """-> list of frame cases, names unique: the blurred own frame, BGR and gray, with the gate, without it, without a margin and at radius 1;
    the sharp own frame among blurred neighbours; one-sided neighbours from the clip's first frame; the gained clip with the gain on and off;
    a fold pair through the occlusion test; a zoomed window; one source alone; the 2 x 2 dense case"""
    h = 37 - 5
    out = [blur_clip("blurred-own", 0, 3), blur_clip("blurred-own", 1, 1), blur_clip("blurred-own", 0, 3, gate_mode=1, name="gate-off"),
           blur_clip("blurred-own", 0, 3, margin=0, strength=255, radius=1, name="no-margin-radius-1"), blur_clip("blurred-own", 2, 3, margin=64, name="margin-64"),
           blur_clip("sharp-own", 0, 3), blur_clip("sharp-own", 1, 1), blur_clip("blurred-own", 3, 3, q=0, radius=3, name="first-frame-radius-3"),
           blur_clip("blurred-own", 0, 3, min_pairs=100000, name="too-few-pairs"),
           _with(dcases.gained_clip(), min_pairs=200, margin=0), _with(dcases.gained_clip(), name="gain-off", gain_mode=1, min_pairs=200, margin=0),
           _with(dcases.from_shutter(scases.fold_clip(37, 67, 1, 1, 0), "fold-visible", 1, radius=1, occlusion=1), min_pairs=200, margin=0, strength=40),
           _with(dcases.from_shutter(scases.fold_clip(37, 67, 3), "fold-zoom", 0, radius=1, window=(2, 3, h, (h * 67) // 37)), min_pairs=1, margin=0, gate_mode=1),
           _with(dcases.from_shutter(scases.smooth_clip(16, 131, 3, 22, t=0.0, shutter=0.0, samples=1, nsources=1), "one-source", 0)),
           _with(dcases.from_shutter(scases.dense_clip(pose_table, "2x2", 2, 2, 3, holes=0.0), "2x2", 1, radius=1), min_pairs=1, margin=0)]
    assert len({c["name"] for c in out}) == len(out)
    return out


sources_and_poses = dcases.sources_and_poses


def run_spec(case, q=None):
    """the definition on frame q of a case.  -> deblur_frame's dict plus sources"""
    src, M, m = sources_and_poses(case, q)
    pick = lambda k: [case[k][n] for n in src]
    r = spec.deblur_frame(pick("frames"), pick("depths"), pick("Rs"), pick("ts"), case["K"], M, m, case["window"], case["strength"], case["margin"], case["min_pairs"],
                          case["gate_mode"], case["min_overlap"], case["gain_mode"], case["occlusion"], case["search"], case["tol_q16"], case["mode"], case["q5_mode"],
                          case["iterations"])
    return dict(r, sources=src)


def abi_margin(case):
    """the case's margin as the C ABI's word: 0 is 'none', -1"""
    return -1 if case["margin"] == 0 else case["margin"]
