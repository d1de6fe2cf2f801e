"""GPU-free tests of the spatial top-up (include/rsdsfm_denoise_spatial.h): the definition's properties on random small frames
(tests/denoise_spatial_spec_numpy.py), the vectorised definition against a loop per pixel written independently of it, a half-supported frame,
the quality scene (a loose floor, the measured ranges printed), the mover scene (what the stage is for), the golden fixture, and the host-only
pieces: the parameter struct, the launch counts, the exported symbols, the refusals that need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import denoise_spatial_cases as cases  # noqa: E402
import denoise_spatial_spec_numpy as spec  # noqa: E402
import denoise_spec_numpy as temporal  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_denoise_spatial_v1.npz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_denoise_spatial.h")).read()  # what this file tests is declared there
NEW_SYMBOLS = {"rsdsfm_denoise_spatial_params_init", "rsdsfm_denoise_spatial_dev", "rsdsfm_denoise_spatial_launches", "rsdsfm_denoise_spatial_frame_dev",
               "rsdsfm_denoise_spatial_frame_launches", "rsdsfm_denoise_spatial_video_dev"}
ERR_INVALID = -1


def _random_frame(rng):
    rows, cols, ch = int(rng.integers(2, 20)), int(rng.integers(2, 70)), int(rng.choice([1, 3]))
    image, mask, weight = cases.frame(rows, cols, ch, seed=int(rng.integers(0, 1000)), set_fraction=float(rng.choice([0.3, 0.8, 1.0])))
    return image, mask, (weight if rng.random() < 0.7 else None), int(rng.integers(1, 256)), int(rng.integers(1, 256)), int(rng.integers(1, 4))


# ---------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------
def test_properties_on_random_frames():
    """200 random frames of 2 .. 19 rows x 2 .. 69 columns, random masks, weights, h, target and S: the counters sum to rows x cols; every output
    byte of a set pixel lies within the min and max of its channel over the set pixels of its (2 S + 1)^2 window; every unset pixel is 0; a pixel
    with n >= target keeps its bytes; the kept pixels are the input's byte for byte; D(p, q) = D(q, p)"""
    rng = np.random.default_rng(11)
    seen = np.zeros(3, dtype=np.int64)
    for it in range(200):
        image, mask, weight, h, target, S = _random_frame(rng)
        r = spec.denoise_spatial(image, mask, weight, h, target, S)
        rows, cols = mask.shape
        I, out = temporal._planes(image).astype(np.int64), temporal._planes(r["image"]).astype(np.int64)
        v = mask != 0
        assert sum(r["counts"]) == rows * cols and r["counts"][0] == int((~v).sum())
        assert (out[~v] == 0).all() and (r["support"][~v] == 0).all()
        window = [(dy, dx) for dy in range(-S, S + 1) for dx in range(-S, S + 1)]
        lo = 255 + np.min([spec._shift(np.where(v[..., None], I, 255) - 255, dy, dx) for dy, dx in window], axis=0)  # 255 where unset or outside
        hi = np.max([spec._shift(np.where(v[..., None], I, 0), dy, dx) for dy, dx in window], axis=0)
        assert (out[v] >= lo[v]).all() and (out[v] <= hi[v]).all(), it
        n = np.where(v, 16, 0) if weight is None else weight.astype(np.int64)
        full = v & (n >= target)
        assert np.array_equal(out[full], I[full]) and np.array_equal(r["support"][full], np.minimum(255, n[full]))
        kept = v & (np.maximum(0, target - n) * r["sum_w"] == 0)
        assert np.array_equal(out[kept], I[kept]) and r["counts"][1] == int(kept.sum())
        dy, dx = spec.displacements(S)[int(rng.integers(0, (2 * S + 1) ** 2 - 1))]
        _, D, N = spec.patch_weight(I, v, dy, dx, h)
        _, Db, Nb = spec.patch_weight(I, v, -dy, -dx, h)
        both = v & spec._shift(v, dy, dx)
        assert np.array_equal(D[both], spec._shift(Db, dy, dx)[both]) and np.array_equal(N[both], spec._shift(Nb, dy, dx)[both]) and (N[both] >= I.shape[2]).all()
        seen += np.array(r["counts"])
    assert (seen > 0).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_a_constant_image_is_unchanged(channels):
    shape = (9, 21) if channels == 1 else (9, 21, 3)
    image = np.full(shape, 137, dtype=np.uint8)
    _, mask, weight = cases.frame(9, 21, channels)
    for S in cases.SEARCHES:
        r = spec.denoise_spatial(image, mask, weight, 1, 255, S)
        keep = (mask != 0) if channels == 1 else (mask != 0)[..., None]
        assert np.array_equal(r["image"], np.where(keep, image, 0)) and r["counts"][2] > 0


def test_the_definition_equals_a_loop_per_pixel():
    """search = 1 (and, on smaller frames, 2 and 3) against denoise_spatial_brute, which shares nothing with the vectorised definition"""
    rng = np.random.default_rng(5)
    for it in range(24):
        image, mask, weight, h, target, S = _random_frame(rng)
        S = 1 if it < 12 else S
        image, mask = image[:10, :24], mask[:10, :24]
        weight = None if weight is None else weight[:10, :24]
        r = spec.denoise_spatial(image, mask, weight, h, target, S)
        img, sup, counts = spec.denoise_spatial_brute(image, mask, weight, h, target, S)
        assert np.array_equal(r["image"], img) and np.array_equal(r["support"], sup) and r["counts"] == counts, (it, S)


@pytest.mark.parametrize("channels", [1, 3])
def test_a_supported_half_keeps_its_bytes(channels):
    image, mask, weight = cases.frame(18, 66, channels, seed=9)
    weight = weight.copy()
    weight[:, :33] = np.maximum(weight[:, :33], 80)
    weight[:, 33:] = np.minimum(weight[:, 33:], 40)
    r = spec.denoise_spatial(image, mask, weight, 40, 80, 2)
    keep = np.where((mask != 0) if channels == 1 else (mask != 0)[..., None], image, 0)
    assert np.array_equal(r["image"][:, :33], keep[:, :33]) and not np.array_equal(r["image"][:, 33:], keep[:, 33:])
    assert np.array_equal(r["support"][:, :33], np.where(mask != 0, weight, 0)[:, :33])


def test_the_defaults_and_the_bounds():
    assert (spec.STRENGTH_DEFAULT, spec.TARGET_DEFAULT, spec.SEARCH_DEFAULT, spec.SEARCH_MAX, spec.B_MIN) == (12, 80, 2, 3, 128)
    sat = np.full((9, 9, 3), 255, dtype=np.uint8)
    r = spec.denoise_spatial(sat, np.ones((9, 9), dtype=np.uint8), np.ones((9, 9), dtype=np.uint8), 1, 255, 3)  # the largest numerator: asserted inside
    assert (r["image"] == 255).all() and r["support"][4, 4] == 255 and r["sum_w"][4, 4] == 768
    r = spec.denoise_spatial(sat, np.ones((9, 9), dtype=np.uint8), np.zeros((9, 9), dtype=np.uint8), 1, 255, 1)  # n = 0: the mean alone
    assert (r["image"] == 255).all() and r["counts"] == [0, 0, 81]
    lone = np.zeros((5, 5), dtype=np.uint8)
    lone[2, 2] = 7
    r = spec.denoise_spatial(sat[:5, :5, 0].copy(), lone, np.zeros((5, 5), dtype=np.uint8), 12, 80, 2)  # no candidate and n = 0: W = 0
    assert r["image"][2, 2] == 255 and r["support"][2, 2] == 0 and r["counts"] == [24, 1, 0]


def test_the_quality_scene_is_denoised():
    """mean absolute error against the clean image relative to the input's, eight seeds, no weight plane, h = 12, target 80: below 0.8 for every
    seed, S and channel count -- a loose floor meaning "it denoises", not a tuned number.  The ranges measured on this definition (printed; DESIGN
    section 12 has them): gray 0.512 - 0.526 / 0.480 - 0.500 / 0.491 - 0.508 and BGR 0.496 - 0.506 / 0.487 - 0.496 / 0.518 - 0.527 at S = 1 / 2 / 3"""
    full = np.ones((cases.QUALITY_ROWS, cases.QUALITY_COLS), dtype=np.uint8)
    for channels in (1, 3):
        for S in cases.SEARCHES:
            ratios = []
            for seed in range(cases.QUALITY_SEEDS):
                clean, noisy = cases.quality_scene(channels, seed)
                out = spec.denoise_spatial(noisy, full, None, 12, 80, S)["image"].reshape(clean.shape).astype(np.int64)
                ratios.append(np.abs(out - clean).mean() / np.abs(noisy.reshape(clean.shape).astype(np.int64) - clean).mean())
            print("quality scene: channels %d S %d ratio %.3f - %.3f" % (channels, S, min(ratios), max(ratios)))
            assert max(ratios) < 0.8, (channels, S, ratios)


def test_the_mover_scene_is_topped_up(rsdsfm):
    """synth.render_sequence's static scene with a mover under noise of +-6 through the temporal definition, then the top-up with the temporal
    weight plane: over the pixels time left with the own frame alone the error against the clean frame falls (measured on this definition: 54
    own-only pixels, mean absolute error 3.31 -> 2.80, ratio 0.845 at the default target; under this noise the temporal weights end at 65, so
    the default target of 80 tops every pixel up, and the ratio over all of them is 0.826), and every pixel with n >= target keeps its temporal
    bytes -- checked at target 56 too, which a third of the frame reaches"""
    sc = cases.mover_scene(rsdsfm.synth)
    t = sc["temporal"]
    own = sc["own_only"]
    assert own.sum() > 0 and (t["weight"] >= 56).sum() > own.sum()
    clean = sc["clean"].astype(np.int64)
    err = lambda img: np.abs(img.astype(np.int64) - clean)[own].mean()
    for target in (spec.TARGET_DEFAULT, 56):
        r = spec.denoise_spatial(t["image"], t["mask"], t["weight"], target=target)
        ratio = err(r["image"]) / err(t["image"])
        print("mover scene, target %d: %d own-only pixels, error %.3f -> %.3f, ratio %.3f" % (target, int(own.sum()), err(t["image"]), err(r["image"]), ratio))
        assert ratio < 1
        full = t["weight"] >= target
        assert np.array_equal(r["image"][full], t["image"][full]) and (r["support"][own] > 16).all() and r["counts"][1] >= int(full.sum())


def test_spec_equals_the_golden_fixture():
    g = np.load(GOLDEN)
    golden = cases.golden_cases()
    assert {k.split("/")[0] for k in g.files} == {c["name"] for c in golden}
    seen = np.zeros(3, dtype=np.int64)
    for case in golden:
        n = case["name"] + "/"
        weight = g[n + "in_weight"] if g[n + "in_weight"].size else None
        assert np.array_equal(g[n + "in_image"], case["image"]) and np.array_equal(g[n + "in_mask"], case["mask"]) and (weight is None) == (case["weight"] is None)
        h, target, S = (int(x) for x in g[n + "params"])
        r = spec.denoise_spatial(g[n + "in_image"], g[n + "in_mask"], weight, h or spec.STRENGTH_DEFAULT, target or spec.TARGET_DEFAULT, S or spec.SEARCH_DEFAULT)
        assert np.array_equal(r["image"], g[n + "image"]) and np.array_equal(r["support"], g[n + "support"]) and r["counts"] == g[n + "counts"].tolist(), n
        seen += np.array(r["counts"])
    assert (seen > 0).all() and os.path.getsize(GOLDEN) <= 32 * 1024


# ---------------------------------------------------------------------------------------------------
# the library's surface
# ---------------------------------------------------------------------------------------------------
def test_the_header_names_its_definition_and_its_symbols():
    assert "tests/denoise_spatial_spec_numpy.py" in HEADER_TEXT and '#include "rsdsfm_denoise.h"' in HEADER_TEXT
    assert '#include "rsdsfm_denoise_spatial.h"' in open(os.path.join(ROOT, "include", "rsdsfm_denoise.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER_TEXT), name
    assert "choices, not measurements" in HEADER_TEXT and "NOT here" in HEADER_TEXT and "d_counts6_or_null" in HEADER_TEXT


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_symbols_are_exported_by_both_builds(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.denoise_spatial_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    assert NEW_SYMBOLS <= set(rsdsfm.declared_symbols()) and not NEW_SYMBOLS & set(rsdsfm.denoise_declared_symbols())
    for name in ("denoise_spatial_dev", "denoise_spatial", "denoise_spatial_frame_dev", "denoise_spatial_video_dev"):
        assert callable(getattr(rsdsfm.Solver, name))
    d = rsdsfm.denoise_spatial_default_params()
    assert (d["strength"], d["target"], d["search"]) == (spec.STRENGTH_DEFAULT, spec.TARGET_DEFAULT, spec.SEARCH_DEFAULT)
    assert ctypes.sizeof(rsdsfm.DenoiseSpatialParams) == 32 and rsdsfm.DENOISE_SPATIAL_SEARCH_MAX == spec.SEARCH_MAX
    p = rsdsfm.DenoiseSpatialParams()
    assert lib.rsdsfm_denoise_spatial_params_init(ctypes.byref(p)) == 0 and p.struct_bytes == 32 and list(p.reserved) == [0, 0, 0, 0]
    assert ctypes.sizeof(rsdsfm.DenoiseParams) == 48  # the temporal struct is as it was


def test_launch_counts_and_host_errors(rsdsfm):
    assert rsdsfm.denoise_spatial_launches() == 1
    for r, c_ in ((2, 2), (37, 67), (720, 1280), (16384, 16384)):
        for n in (1, 2, 5, 15):
            assert rsdsfm.denoise_spatial_frame_launches(r, c_, n) == rsdsfm.denoise_launches(r, c_, n) + 1
        for n in (0, -1, 16):
            with pytest.raises(rsdsfm.RsdsfmError):
                rsdsfm.denoise_spatial_frame_launches(r, c_, n)
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.denoise_spatial_frame_launches(r, c_, 2)
    lib = rsdsfm.load_library()
    i32, f64 = ctypes.c_int32, ctypes.c_double
    assert lib.rsdsfm_denoise_spatial_params_init(None) == ERR_INVALID
    # no context: refused before anything is read
    assert lib.rsdsfm_denoise_spatial_dev(None, None, None, None, i32(3), i32(8), i32(8), i32(0), i32(0), i32(0), None, None, None) == ERR_INVALID
    assert lib.rsdsfm_denoise_spatial_frame_dev(None, None, i32(3), None, None, None, f64(1), f64(1), f64(0), f64(0), i32(8), i32(8), 0, 0, i32(0), i32(1), None, None, None,
                                                None, None, None, None, None, None, None) == ERR_INVALID
    assert lib.rsdsfm_denoise_spatial_video_dev(None, None, i32(1), i32(8), i32(8), i32(3), f64(1), f64(1), f64(0), f64(0), None, None, None, None, None, None, None, None, 0,
                                                0, i32(0), None, None, None, None, None, None, None, None) == ERR_INVALID
