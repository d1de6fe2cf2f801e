"""GPU-free tests of the sharpness transfer (include/rsdsfm_deblur.h): the definition (tests/deblur_spec_numpy.py) against a second, loop-form
transcription and against its golden fixture, its consequences (every tau 0: the own frame; the order of the layers; tau 16: u = w; a sharp
frame among blurred neighbours), tau's branches against the library's host function, what the stage is for on the blurred shift scene, the
library's surface, the launch counts and the synthetic blur."""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import deblur_cases as cases  # noqa: E402
import deblur_spec_numpy as spec  # noqa: E402
import denoise_spec_numpy as dn  # noqa: E402
from make_golden_deblur import digest  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_deblur_v1.npz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_deblur.h")).read()  # what this file tests is declared there: without the header, nothing here runs
NEW_SYMBOLS = {"rsdsfm_deblur_params_init", "rsdsfm_deblur_sharpness_dev", "rsdsfm_deblur_tau", "rsdsfm_deblur_accumulate_dev", "rsdsfm_deblur_frame_dev",
               "rsdsfm_deblur_launches", "rsdsfm_deblur_video_dev"}
ERR_INVALID = -1


# ---------------------------------------------------------------------------------------------------
# the definition, a second time: loops over pixels, Python integers
# ---------------------------------------------------------------------------------------------------
def _loop_deblur(ref, rmask, layers, records, min_overlap, gain_mode, strength, margin, min_pairs, gate_mode):
    rows, cols = rmask.shape
    R = ref.reshape(rows, cols, -1)
    ch = R.shape[2]
    cells = [[None] * cols for _ in range(rows)]
    for y in range(rows):
        for x in range(cols):
            cells[y][x] = [16 * int(b) for b in R[y, x]] + [16] if rmask[y, x] else [0] * (ch + 1)
    sharps, taus = [], []
    for j, (limg, lmask) in enumerate(layers):
        L = limg.reshape(rows, cols, -1)
        G = dn.gains(records[j] if records else None, ch, min_overlap, gain_mode)
        k = [[[min(255, (int(G[c]) * int(L[y, x, c]) + 32768) >> 16) for c in range(ch)] for x in range(cols)] for y in range(rows)]
        v = [[bool(rmask[y, x]) and bool(lmask[y, x]) for x in range(cols)] for y in range(rows)]
        yr = [[sum(int(b) for b in R[y, x]) for x in range(cols)] for y in range(rows)]
        yl = [[sum(k[y][x]) for x in range(cols)] for y in range(rows)]
        pairs = a_r = a_l = 0
        for y in range(rows):
            for x in range(cols):
                for qy, qx in ((y, x + 1), (y + 1, x)):
                    if v[y][x] and qy < rows and qx < cols and v[qy][qx]:
                        pairs += 1
                        a_r += (yr[y][x] - yr[qy][qx]) ** 2
                        a_l += (yl[y][x] - yl[qy][qx]) ** 2
        sharps.append([pairs, a_r, a_l, 0])
        if pairs < min_pairs or 16 * a_l <= (16 + margin) * a_r:
            t = 0
        else:
            t = min(32, (16 * (a_l - a_r)) // max(a_r, 1))
        taus.append(t)
        for y in range(rows):
            for x in range(cols):
                if not v[y][x]:
                    continue
                d = n = 0
                for py in range(max(y - 1, 0), min(y + 2, rows)):
                    for px in range(max(x - 1, 0), min(x + 2, cols)):
                        if v[py][px]:
                            d += yr[py][px] - yl[py][px]
                            n += ch
                w = 16 if gate_mode == 1 else 16 - min(16, (16 * abs(d)) // (strength * n))
                u = (w * t + 8) >> 4
                for c in range(ch):
                    cells[y][x][c] += u * k[y][x][c]
                cells[y][x][ch] += u
    image = np.zeros((rows, cols, ch), dtype=np.uint8)
    weight = np.zeros((rows, cols), dtype=np.uint8)
    for y in range(rows):
        for x in range(cols):
            n = cells[y][x][ch]
            weight[y, x] = n
            if n:
                image[y, x] = [(2 * s + n) // (2 * n) for s in cells[y][x][:ch]]
    counts = [int((weight == 0).sum()), int((weight == 16).sum()), int((weight > 16).sum())]
    return dict(image=image.reshape(ref.shape), mask=(weight > 0).astype(np.uint8), weight=weight, counts=counts, sharps=sharps, taus=taus)


@pytest.mark.parametrize("channels", [1, 3])
def test_spec_equals_a_loop_form_transcription(channels):
    """random cases: sizes 2 x 2 .. 9 x 11, one to three layers around a blurred or a plain reference, masks with holes, overlap records that give
    a gain, both gate modes, margins 0 .. 64, min_pairs below and above the pairs there are"""
    rng = np.random.default_rng(77 + channels)
    seen = set()
    for trial in range(24):
        rows, cols = int(rng.integers(2, 10)), int(rng.integers(2, 12))
        blurred, rmask, sharp = cases.blurred_reference(rows, cols, channels, seed=trial, width=3)
        ref = blurred if trial % 3 else sharp
        ls = cases.layers(sharp, rows, cols, channels, 1 + trial % 3, seed=trial)
        recs = [list(cases.records(channels).values())[(trial + j) % 5] for j in range(len(ls))] if trial % 2 else None
        kw = dict(min_overlap=int(rng.choice([1, 1024, 6000])), gain_mode=int(trial % 5 == 0), strength=int(rng.choice([1, 7, 24, 255])), margin=int(rng.choice([0, 4, 64])),
                  min_pairs=int(rng.choice([1, 30])), gate_mode=int(trial % 4 == 3))
        want = _loop_deblur(ref, rmask, ls, recs, **kw)
        got = spec.deblur(ref, rmask, ls, recs, None, **kw)
        for k in ("image", "mask", "weight"):
            assert np.array_equal(got[k], want[k]), (trial, k)
        assert got["counts"] == want["counts"] and got["taus"] == want["taus"] and got["sharps"].tolist() == want["sharps"], trial
        seen |= set(want["taus"])
    assert 0 in seen and 32 in seen and len(seen) >= 4, seen


def test_spec_equals_the_golden_fixture(oracle):
    g = np.load(GOLDEN)
    all_cases = cases.all_cases(oracle.pose_table)
    assert {k.split("/")[0] for k in g.files} == {c["name"] for c in all_cases}
    seen, taus = np.zeros(3, dtype=np.int64), set()
    for case in all_cases:
        n = case["name"] + "/"
        assert digest(case) == int(g[n + "digest"]), n
        r = cases.run_spec(case)
        for k in ("image", "mask", "weight", "records", "sharps"):
            assert np.array_equal(r[k], g[n + k]), (n, k)
        assert list(r["counts"]) == g[n + "counts"].tolist() and sum(r["counts"]) == r["mask"].size and r["taus"] == g[n + "taus"].tolist(), n
        seen += np.array(r["counts"])
        taus |= set(r["taus"])
    assert (seen > 0).all() and {0, 32} < taus
    assert os.path.getsize(GOLDEN) <= 128 * 1024
    assert {c["frames"][0].ndim for c in all_cases} == {2, 3} and {c["occlusion"] for c in all_cases} == {0, 1} and {c["gate_mode"] for c in all_cases} == {0, 1}
    assert {len(cases.sources_and_poses(c)[0]) for c in all_cases} >= {1, 2, 3, 4, 5}
    assert not np.array_equal(g["gained/image"], g["gain-off/image"]) and not np.array_equal(g["blurred-own-bgr-0/image"], g["gate-off/image"])


# ---------------------------------------------------------------------------------------------------
# consequences
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
def test_every_tau_zero_returns_the_own_frame(channels):
    """(a) layers that are no sharper (the reference's own bytes under other masks, and softer copies): the reference's bytes and mask exactly"""
    ref, rmask = cases.reference(17, 65, channels)
    soft = spec.box_blur(ref, 5)
    ls = [(ref, cases.reference(17, 65, channels, seed=1)[1]), (soft, np.ones((17, 65), dtype=np.uint8))]
    r = spec.deblur(ref, rmask, ls, min_pairs=1)
    on = rmask != 0
    keep = on if channels == 1 else on[..., None]
    assert r["taus"] == [0, 0]
    assert np.array_equal(r["image"], np.where(keep, ref, 0)) and np.array_equal(r["mask"], on.astype(np.uint8))
    assert np.array_equal(r["weight"], 16 * on) and r["counts"] == [int((~on).sum()), int(on.sum()), 0]
    none = spec.deblur(ref, rmask, [])
    assert np.array_equal(none["image"], r["image"]) and np.array_equal(none["weight"], r["weight"]) and none["counts"] == r["counts"]


@pytest.mark.parametrize("channels", [1, 3])
def test_the_result_does_not_depend_on_the_order_of_three_layers(channels):
    """(b)"""
    blurred, rmask, sharp = cases.blurred_reference(37, 67, channels)
    ls = cases.layers(sharp, 37, 67, channels, 3)
    recs = [cases.records(channels)[k] for k in ("plain", "small", "zero")]
    sharps = [cases.sharp_records()[k][0] for k in ("half", "thirty", "twice")]  # three different factors
    want = spec.deblur(blurred, rmask, ls, recs, sharps, strength=60)
    assert want["taus"] == [8, 30, 16] and want["counts"][2] > 0 and len(np.unique(want["weight"])) > 20
    for perm in itertools.permutations(range(3)):
        got = spec.deblur(blurred, rmask, [ls[i] for i in perm], [recs[i] for i in perm], [sharps[i] for i in perm], strength=60)
        for k in ("image", "mask", "weight"):
            assert np.array_equal(got[k], want[k]), perm
        assert got["counts"] == want["counts"] and got["taus"] == [want["taus"][i] for i in perm]


def test_tau_16_counts_the_gate_itself():
    """(c) u = (16 w + 8) >> 4 = w: a step with the record `twice` adds exactly the gate"""
    blurred, rmask, sharp = cases.blurred_reference(33, 129, 3)
    (layer, lmask), = cases.layers(sharp, 33, 129, 3, 1)
    T, t = cases.sharp_records()["twice"]
    assert t == 16 == spec.tau(T)
    r = spec.deblur(blurred, rmask, [(layer, lmask)], None, [T], strength=40)
    v, YR, YL, _ = spec.lumas(blurred, rmask, layer, lmask, dn.gains(None, 3))
    w = spec.gate(v, YR, YL, 3, 40)
    assert np.array_equal(r["weight"], 16 * (rmask != 0) + w) and len(np.unique(w)) >= 10
    for name, (T, t) in cases.sharp_records().items():  # every u of every tau
        u = (np.arange(17) * t + 8) >> 4
        assert u[0] == 0 and u[16] == t and (np.diff(u) >= 0).all(), name


# ---------------------------------------------------------------------------------------------------
# tau
# ---------------------------------------------------------------------------------------------------
def test_tau_of_every_record_case_and_the_host_function(rsdsfm):
    recs = cases.sharp_records()
    assert {t for _, t in recs.values()} >= {0, 4, 8, 16, 30, 31, 32}
    for name, (T, t) in recs.items():
        assert spec.tau(T) == t, name
        assert rsdsfm.deblur_tau(T) == t and rsdsfm.deblur_tau(T, 4, 1024) == t, name
        for word in (-1, 1, 16, 64):
            for min_pairs in (1, 1023, 1024, 1025, 5001, 2 ** 40):
                assert rsdsfm.deblur_tau(T, word, min_pairs) == spec.tau(T, spec.margin_value(word), min_pairs), (name, word, min_pairs)
    # the margin: a sixteenth more or less decides at A_L = 1.25 A_R
    T = recs["margin"][0]
    assert spec.tau(T, 3) == 4 and spec.tau(T, 4) == 0 and spec.tau(T, 0) == 4 and spec.tau(recs["equal"][0], 0) == 0
    assert spec.margin_value(-1) == 0 and spec.margin_value(0) == spec.MARGIN_DEFAULT == 4 and spec.margin_value(64) == 64
    lib = rsdsfm.load_library()
    out = ctypes.c_int32(7)
    p = T.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, 0, 0, ctypes.byref(out)), (p, 0, 0, None), (p, -2, 0, ctypes.byref(out)), (p, 65, 0, ctypes.byref(out)), (p, 0, -1, ctypes.byref(out))):
        assert lib.rsdsfm_deblur_tau(args[0], ctypes.c_int32(args[1]), ctypes.c_int64(args[2]), args[3]) == ERR_INVALID
    assert out.value == 7
    with pytest.raises(rsdsfm.RsdsfmError):
        rsdsfm.deblur_tau(T, 65)


def test_the_sharpness_record_counts_every_adjacent_pair_once():
    """a full 4 x 5 gray frame has 4 * 4 + 3 * 5 = 31 pairs; a hole takes its (up to) four pairs away; a ramp of slope 3 along the rows gives 9
    per horizontal pair and 0 per vertical one; both images are summed on the same support"""
    ramp = (3 * np.arange(5))[None, :].repeat(4, axis=0).astype(np.uint8)
    flat = np.full((4, 5), 9, dtype=np.uint8)
    full = np.ones((4, 5), dtype=np.uint8)
    assert spec.sharpness(ramp, full, flat, full).tolist() == [31, 16 * 9, 0, 0] and spec.sharpness(flat, full, ramp, full).tolist() == [31, 0, 16 * 9, 0]
    hole = full.copy()
    hole[1, 2] = 0
    assert spec.sharpness(ramp, full, ramp, hole).tolist() == [27, 14 * 9, 14 * 9, 0] and spec.sharpness(ramp, hole, ramp, full).tolist() == [27, 14 * 9, 14 * 9, 0]
    bgr = np.stack([ramp, ramp, ramp], axis=-1)
    assert spec.sharpness(bgr, full, bgr, full, np.array([5000, 100, 100, 100, 200, 200, 200, 0], dtype=np.uint64)).tolist() == [31, 16 * 81, 4 * 90, 0]
    # (gain 1 / 2, k = (L + 1) >> 1: a row's 0, 3, 6, 9, 12 becomes 0, 2, 3, 5, 6, three channels: steps of 6, 3, 6, 3 in Y_L, 90 per row)


# ---------------------------------------------------------------------------------------------------
# what it is for
# ---------------------------------------------------------------------------------------------------
def _errors(case):
    r = cases.run_spec(case)
    q = case["q"]
    cols_ok = cases.shift_seen_by_all(case)
    clean = case["clean"][q].astype(np.int64)
    assert (r["mask"] == 1).all() and np.array_equal(r["ref"][0], case["frames"][q])  # the own render is the own frame: the renders align exactly
    err = lambda img: np.abs(img.astype(np.int64) - clean)[:, cols_ok].mean()
    return r, err(case["frames"][q]), err(r["image"])


@pytest.mark.parametrize("channels", [3, 1])
def test_a_blurred_frame_among_sharp_neighbours_gets_sharper(channels):
    """the shift scene with its middle frame blurred by a 5-column box, noise +-6 everywhere, K = 2, h = 24: every neighbour's tau > 0 (a condition
    of the inputs), and over the columns all five frames see the mean absolute error against the clean SHARP frame is strictly below the own
    frame's.  Measured on the definition: own 41.2 - 43.3, output 5.6 - 9.4 (ratios 0.13 - 0.22, the gray frames at the upper end); with the
    gate off 0.115 on BGR seed 0.  No ratio other than < 1 is asserted"""
    for seed in range(3):
        r, own, out = _errors(cases.blur_clip("blurred-own", seed, channels))
        print("blurred own, %s, seed %d: taus %s, error %.3f -> %.3f (ratio %.3f)" % ("BGR" if channels == 3 else "gray", seed, r["taus"], own, out, out / own))
        assert len(r["taus"]) == 4 and min(r["taus"]) > 0, r["taus"]
        assert out < own, (own, out)
        assert r["counts"][2] > 0


@pytest.mark.parametrize("channels", [3, 1])
def test_a_sharp_frame_among_blurred_neighbours_keeps_its_bytes(channels):
    """(d) every frame but the own blurred: every tau = 0 and the output is the own frame byte for byte"""
    for seed in range(3):
        case = cases.blur_clip("sharp-own", seed, channels)
        r, own, out = _errors(case)
        assert r["taus"] == [0, 0, 0, 0] and np.array_equal(r["image"], case["frames"][case["q"]]) and (r["weight"] == 16).all() and own == out
        assert r["counts"] == [0, r["mask"].size, 0]


# ---------------------------------------------------------------------------------------------------
# the library's surface
# ---------------------------------------------------------------------------------------------------
def test_the_header_names_its_definition_and_its_symbols():
    assert "tests/deblur_spec_numpy.py" in HEADER_TEXT and '#include "rsdsfm_denoise.h"' in HEADER_TEXT
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER_TEXT), name
    assert "RSDSFM_DEBLUR_LAYERS_MAX 7" in HEADER_TEXT and "NOT here" in HEADER_TEXT and "choices, not measurements" in HEADER_TEXT


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_symbols_are_exported_by_both_builds(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    assert NEW_SYMBOLS <= set(rsdsfm.declared_symbols())
    assert not [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not NEW_SYMBOLS & set(rsdsfm.denoise_declared_symbols())
    for name in ("deblur_sharpness_dev", "deblur_sharpness", "deblur_accumulate_dev", "deblur_accumulate", "deblur_frame_dev", "deblur_video_dev"):
        assert callable(getattr(rsdsfm.Solver, name))
    assert os.path.basename(rsdsfm.DEBLUR_HEADER_PATH) == "rsdsfm_deblur.h"
    d = rsdsfm.deblur_default_params()
    assert (d["radius"], d["strength"], d["margin"], d["min_overlap"], d["min_pairs"], d["gate_mode"], d["gain_mode"], d["occlusion"]) == \
        (spec.RADIUS_DEFAULT, spec.STRENGTH_DEFAULT, spec.MARGIN_DEFAULT, spec.MIN_OVERLAP_DEFAULT, spec.MIN_PAIRS_DEFAULT, 0, 0, 0)
    assert ctypes.sizeof(rsdsfm.DeblurParams) == 64 and rsdsfm.DEBLUR_LAYERS_MAX == spec.LAYERS_MAX and rsdsfm.DEBLUR_RADIUS_MAX == spec.RADIUS_MAX
    assert rsdsfm.DEBLUR_TAU_MAX == spec.TAU_MAX and rsdsfm.DEBLUR_TAUS_PER_FRAME == 2 * spec.RADIUS_MAX
    p = rsdsfm.DeblurParams()
    assert lib.rsdsfm_deblur_params_init(ctypes.byref(p)) == 0 and p.struct_bytes == 64 and list(p.reserved) == [0, 0, 0, 0]


def test_launch_counts_and_host_errors(rsdsfm):
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385), (0, 0)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.deblur_launches(r, c_, 2)
    for r, c_ in ((2, 2), (37, 67), (720, 1280), (16384, 16384)):
        one = rsdsfm.stabilize_window_launches(r, c_)
        assert rsdsfm.deblur_launches(r, c_, 1) == one + 1
        for n in (2, 3, 5, 8):
            assert rsdsfm.deblur_launches(r, c_, n) == n * one + 3 * (n - 1) == rsdsfm.denoise_launches(r, c_, n) + (n - 1)
        for n in (0, -1, 9):
            with pytest.raises(rsdsfm.RsdsfmError):
                rsdsfm.deblur_launches(r, c_, n)
    lib = rsdsfm.load_library()
    i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert lib.rsdsfm_deblur_params_init(None) == ERR_INVALID
    # no context: refused before anything is read
    assert lib.rsdsfm_deblur_sharpness_dev(None, None, None, None, None, i32(3), i32(8), i32(8), None, i64(0), i32(0), None) == ERR_INVALID
    assert lib.rsdsfm_deblur_accumulate_dev(None, None, None, None, None, i32(3), i32(8), i32(8), None, i64(0), i32(0), i32(24), None, i32(0), i64(0), i32(0), None, i32(1),
                                            i32(1), None, None, None, None) == ERR_INVALID
    assert lib.rsdsfm_deblur_frame_dev(None, None, i32(3), None, None, None, f64(1), f64(1), f64(0), f64(0), i32(8), i32(8), 0, 0, i32(0), i32(1), None, None, None, None,
                                       None, None, None, None, None) == ERR_INVALID
    assert lib.rsdsfm_deblur_video_dev(None, None, i32(1), i32(8), i32(8), i32(3), f64(1), f64(1), f64(0), f64(0), None, None, None, None, None, None, None, None, 0, 0,
                                       i32(0), None, None, None, None, None, None, None) == ERR_INVALID


def test_evaluate_takes_the_keyword(rsdsfm):
    import inspect

    assert inspect.signature(rsdsfm.evaluate.evaluate_real_sequence).parameters["deblur"].default is None
    for value in (True, 2, (2, 24)):
        with pytest.raises(ValueError, match="stabilize"):
            rsdsfm.evaluate.evaluate_real_sequence(None, [], deblur=value)


def test_synthetic_blur_is_a_rounded_box_mean_and_off_by_default(rsdsfm):
    synth = rsdsfm.synth
    v, w, k = synth.default_motion()
    K = (60.0, 60.0, 24.0, 16.0)
    plain, flow, mask = synth.render_sequence(3, 32, 48, K, v, w, k)
    off, flow0, mask0 = synth.render_sequence(3, 32, 48, K, v, w, k, blur=None)
    assert np.array_equal(off, plain) and np.array_equal(flow0, flow) and np.array_equal(mask0, mask)
    ones = synth.render_sequence(3, 32, 48, K, v, w, k, blur=[1, 1, 1])
    assert np.array_equal(ones[0], plain) and np.array_equal(ones[1], flow) and np.array_equal(ones[2], mask)
    b, flow1, mask1 = synth.render_sequence(3, 32, 48, K, v, w, k, blur=[1, 5, 3])
    assert np.array_equal(flow1, flow) and np.array_equal(mask1, mask) and np.array_equal(b[0], plain[0]) and b.dtype == np.uint8 and b.shape == plain.shape
    for j, width in ((1, 5), (2, 3)):
        assert np.array_equal(b[j], spec.box_blur(plain[j], width)) and not np.array_equal(b[j], plain[j])
        h = width // 2
        p = plain[j].astype(np.int64)
        x = 20
        exact = p[:, x - h:x + h + 1].sum(axis=1)  # an interior column: the mean of `width` columns, rounded half up
        assert np.array_equal(b[j][:, x], (2 * exact + width) // (2 * width))
        assert np.array_equal(b[j][:, 0], (2 * ((h + 1) * p[:, 0] + p[:, 1:h + 1].sum(axis=1)) + width) // (2 * width))  # the edge is replicated
    # with speeds (the other render loop), before the noise and after the mover
    sp = synth.render_sequence(3, 32, 48, K, v, w, k, speeds=[1.0, 1.5], blur=[3, 1, 1])[0]
    assert np.array_equal(sp[0], spec.box_blur(synth.render_sequence(3, 32, 48, K, v, w, k, speeds=[1.0, 1.5])[0][0], 3))
    mv = (4, 5, 6, 7, 2, 1)
    moved = synth.render_sequence(3, 32, 48, K, v, w, k, mover=mv)[0]
    both = synth.render_sequence(3, 32, 48, K, v, w, k, mover=mv, blur=[1, 7, 1], noise=4, noise_seed=3)[0]
    d = both[1].astype(np.int64) - spec.box_blur(moved[1], 7)
    assert np.abs(d).max() <= 4 and np.abs(d).max() > 0
    for bad in ([1, 5], [1, 2, 1], [0, 1, 1], [1, 1, -3]):
        with pytest.raises(ValueError):
            synth.render_sequence(3, 32, 48, K, v, w, k, blur=bad)
