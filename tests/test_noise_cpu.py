"""GPU-free tests of the noise level (include/rsdsfm_noise.h): the definition (tests/noise_spec_numpy.py) against the golden fixture and against
a loop per pixel written independently of it, its properties (the histogram sums to n, m is monotone in q, constants and ramps are annihilated,
a constant image gives h = 1), the quality scene (sigma_hat / sigma_true, h = 12 at the project's noise, what the estimated h buys at +-20; loose
floors, the measured values printed), and the host-only pieces: the strength, the parameter struct, the launch counts, the exported symbols,
the refusals that need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import denoise_spec_numpy as temporal  # noqa: E402
import noise_cases as cases  # noqa: E402
import noise_spec_numpy as spec  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_noise_v1.npz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_noise.h")).read()
NEW_SYMBOLS = {"rsdsfm_noise_params_init", "rsdsfm_noise_level_dev", "rsdsfm_noise_level_launches", "rsdsfm_noise_strength", "rsdsfm_denoise_accumulate_auto_dev",
               "rsdsfm_denoise_spatial_auto_dev", "rsdsfm_denoise_auto_frame_dev", "rsdsfm_denoise_auto_frame_launches", "rsdsfm_denoise_auto_video_dev"}
ERR_INVALID = -1


# ---------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------
def test_spec_equals_the_golden_fixture():
    g = np.load(GOLDEN)
    golden = cases.golden_cases()
    assert {k.split("/")[0] for k in g.files} == {c["name"] for c in golden}
    assert {c["kind"] for c in golden} == set(cases.KINDS) and {c["quantile_q8"] for c in golden} == set(cases.QUANTILES)
    for case in golden:
        n = case["name"] + "/"
        assert np.array_equal(g[n + "in_image"], case["image"]) and np.array_equal(g[n + "in_mask"], case["mask"]) and int(g[n + "quantile"][0]) == case["quantile_q8"]
        r = spec.noise_level(g[n + "in_image"], g[n + "in_mask"], int(g[n + "quantile"][0]))
        hist = np.zeros(spec.BINS, dtype=np.uint32)
        hist[g[n + "bins"]] = g[n + "counts"]
        assert np.array_equal(r["hist"], hist) and np.array_equal(r["record"], g[n + "record"]), n
    assert os.path.getsize(GOLDEN) <= 32 * 1024


def _brute(image, mask, q):
    """a loop per pixel, sharing nothing with the vectorised definition -> (hist as a list, [n, m, sigma_q8, 0])"""
    img = np.asarray(image)
    rows, cols = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    px = lambda y, x, c: int(img[y, x]) if img.ndim == 2 else int(img[y, x, c])
    hist = [0] * 1024
    for y in range(1, rows - 1):
        for x in range(1, cols - 1):
            if any(mask[y + dy, x + dx] == 0 for dy in (-1, 0, 1) for dx in (-1, 0, 1)):
                continue
            for c in range(ch):
                nine = [px(y + dy, x + dx, c) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
                if min(nine) < 1 or max(nine) > 254:
                    continue
                r = nine[0] - 2 * nine[1] + nine[2] - 2 * nine[3] + 4 * nine[4] - 2 * nine[5] + nine[6] - 2 * nine[7] + nine[8]
                hist[min(abs(r), 1023)] += 1
    n = sum(hist)
    m = 0
    if n:
        k = max(1, (n * (q or 128) + 255) // 256)
        cum = 0
        for b in range(1024):
            cum += hist[b]
            if cum >= k:
                m = b
                break
    return hist, [n, m, (256000 * m + 2023) // 4047, 0]


def test_the_definition_equals_a_loop_per_pixel():
    every = cases.primitive_cases()
    picked = [c for c in every if c["image"].shape[0] * c["image"].shape[1] <= 18 * 66]
    assert len(picked) >= 40 and {c["kind"] for c in picked} == set(cases.KINDS)
    for case in picked:
        r = cases.run_spec(case)
        hist, record = _brute(case["image"], case["mask"], case["quantile_q8"])
        assert r["hist"].tolist() == hist and r["record"].tolist() == record, case["name"]


def test_the_histogram_sums_to_n_and_m_is_monotone_in_q():
    for case in cases.primitive_cases():
        hist = spec.histogram(case["image"], case["mask"])
        ms = []
        for q in range(1, 257, 5):
            rec = spec.resolve(hist, q)
            assert int(rec[0]) == int(hist.astype(np.int64).sum()) and int(rec[3]) == 0 and int(rec[2]) == (256000 * int(rec[1]) + 2023) // 4047
            ms.append(int(rec[1]))
        assert ms == sorted(ms), case["name"]
        if int(hist.sum()):
            nz = np.nonzero(hist)[0]
            assert int(spec.resolve(hist, 256)[1]) == nz[-1] and int(spec.resolve(hist, 1)[1]) >= nz[0]  # k = n: the largest; k = ceil(n / 256)
            assert int(hist.sum()) > 256 or int(spec.resolve(hist, 1)[1]) == nz[0]  # k = 1: the smallest
        else:
            assert ms == [0] * len(ms)
        assert np.array_equal(spec.resolve(hist, 0), spec.resolve(hist, 128))


@pytest.mark.parametrize("channels", [1, 3])
def test_constants_and_ramps_are_annihilated(channels):
    """adding a constant, a ramp in x, in y and an xy term (nothing clips) leaves the histogram as it is"""
    rng = np.random.default_rng(3)
    rows, cols = 19, 37
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    image = rng.integers(60, 100, size=shape)
    mask = np.where(rng.random((rows, cols)) < 0.9, 3, 0).astype(np.uint8)
    y, x = np.mgrid[0:rows, 0:cols]
    base = spec.histogram(image.astype(np.uint8), mask)
    assert base.sum() > 0
    for add in (40 + 0 * x, 2 * x, 3 * y, 2 * x + 3 * y + 7):
        a = add if channels == 1 else add[..., None]
        moved = image + a
        assert moved.min() >= 1 and moved.max() <= 254
        assert np.array_equal(spec.histogram(moved.astype(np.uint8), mask), base)
    small = rng.integers(100, 110, size=(9, 9))
    ys, xs = np.mgrid[0:9, 0:9]
    assert np.array_equal(spec.histogram((small + xs * ys).astype(np.uint8), np.ones((9, 9), dtype=np.uint8)), spec.histogram(small.astype(np.uint8), np.ones((9, 9), dtype=np.uint8)))


def test_a_constant_image_asks_for_the_smallest_strength():
    image = np.full((40, 40, 3), 137, dtype=np.uint8)
    r = spec.noise_level(image, np.ones((40, 40), dtype=np.uint8))
    assert r["record"].tolist() == [3 * 38 * 38, 0, 0, 0] and int(r["hist"][0]) == 3 * 38 * 38
    assert spec.noise_strength(int(r["record"][0]), int(r["record"][1])) == 1
    sat = np.full((40, 40), 255, dtype=np.uint8)  # a saturated flat area has no sample: it cannot pull the estimate to 0
    assert spec.noise_level(sat, np.ones((40, 40), dtype=np.uint8))["record"].tolist() == [0, 0, 0, 0]
    assert spec.noise_level(image[:2], np.ones((2, 40), dtype=np.uint8))["record"].tolist() == [0, 0, 0, 0]  # two rows: no candidate


# ---------------------------------------------------------------------------------------------------
# quality
# ---------------------------------------------------------------------------------------------------
def _ratio(clean, frames, h):
    full = np.ones(clean.shape[:2], dtype=np.uint8)
    mid = frames[2]
    out = temporal.denoise(mid, full, [(f, full) for k, f in enumerate(frames) if k != 2], strength=h)["image"]
    err = lambda img: np.abs(img.reshape(clean.shape).astype(np.int64) - clean).mean()
    return err(out) / err(mid)


def test_the_estimate_follows_the_noise_on_the_quality_scene():
    """the 96 x 130 quality scene, eight seeds, uniform integer noise +-a: sigma_hat / sigma_true within [0.9, 1.2] for a in 2 .. 20 (the measured
    ranges are printed; DESIGN section 12 has them) and h = 12 exactly at the project's a = 6, for both channel counts"""
    for channels in (1, 3):
        for a in cases.AMPLITUDES:
            ratios, hs = [], []
            for seed in range(cases.QUALITY_SEEDS):
                _, frames = cases.quality_clip(channels, seed, a)
                rec = spec.noise_level(frames[2], np.ones(frames[2].shape[:2], dtype=np.uint8))["record"]
                ratios.append(spec.sigma(rec) / cases.sigma_true(a))
                hs.append(spec.noise_strength(int(rec[0]), int(rec[1])))
            print("quality scene: channels %d a %2d sigma_hat / sigma_true %.3f - %.3f, h %d - %d" % (channels, a, min(ratios), max(ratios), min(hs), max(hs)))
            assert 0.9 <= min(ratios) and max(ratios) <= 1.2, (channels, a, ratios)
            if a == 6:
                assert set(hs) == {12}, (channels, hs)


def test_the_estimated_strength_denoises_where_the_default_does_not():
    """five static frames at +-20, the middle one denoised with its four neighbours: mean absolute error against the clean frame relative to the
    input's below 0.6 with the estimated h and above 0.8 with h = 12, every seed, both channel counts"""
    for channels in (1, 3):
        auto, fixed, hs = [], [], []
        for seed in range(cases.QUALITY_SEEDS):
            clean, frames = cases.quality_clip(channels, seed, 20)
            rec = spec.noise_level(frames[2], np.ones(frames[2].shape[:2], dtype=np.uint8))["record"]
            h = spec.noise_strength(int(rec[0]), int(rec[1]))
            hs.append(h)
            auto.append(_ratio(clean, frames, h))
            fixed.append(_ratio(clean, frames, 12))
        print("quality clip at +-20: channels %d estimated h %d - %d ratio %.3f - %.3f, h = 12 ratio %.3f - %.3f" % (channels, min(hs), max(hs), min(auto), max(auto), min(fixed),
                                                                                                               max(fixed)))
        assert max(auto) < 0.6 and min(fixed) > 0.8, (channels, auto, fixed)


# ---------------------------------------------------------------------------------------------------
# the library's surface
# ---------------------------------------------------------------------------------------------------
def test_the_strength_and_its_refusals(rsdsfm):
    lib = rsdsfm.load_library()
    f = rsdsfm.noise_strength
    assert (spec.SCALE_DEFAULT, spec.MIN_SAMPLES_DEFAULT, spec.QUANTILE_DEFAULT, spec.BINS) == (12, 1024, 128, 1024)
    assert f(1024, 16) == 12 and f(1023, 16) == 12 and f(1023, 16, fallback=40) == 40 and f(1024, 16, fallback=40) == 12
    assert f(5000, 0) == 1 and f(5000, 1) == 1 and f(5000, 2) == 2 and f(5000, 339) == 254 and f(5000, 340) == 255 and f(5000, 1023) == 255
    assert f(5000, 16, scale=255) == 255 and f(5000, 16, scale=1) == 1 and f(5000, 24, scale=1) == 2 and f(0, 16, min_samples=0) == 12
    assert f(5, 16, min_samples=5) == 12 and f(4, 16, fallback=7, min_samples=5) == 7 and f(2 ** 40, 16) == 12 and f(5000, 2 ** 40) == 255
    assert f(5000, 1024, scale=1) == 64 and f(5000, 1100, scale=2) == 138 and f(5000, 4071, scale=1) == 254 and f(5000, 4072, scale=1) == 255 and f(5000, 4096, scale=1) == 255
    rng = np.random.default_rng(2)
    for it in range(600):
        n, m = int(rng.integers(0, 5000)), int(rng.integers(0, 1100 if it % 2 else 5000))
        scale, fb, ms = int(rng.integers(0, 256 if it % 3 else 4)), int(rng.integers(1, 256)), int(rng.integers(0, 3000))
        assert f(n, m, scale, fb, ms) == spec.noise_strength(n, m, scale, fb, ms), (n, m, scale, fb, ms)
    for bad in (dict(n=-1), dict(m=-1), dict(scale=256), dict(scale=-1), dict(fallback=256), dict(fallback=-1), dict(min_samples=-1)):
        with pytest.raises(rsdsfm.RsdsfmError):
            f(**dict(dict(n=5000, m=16), **bad))
    assert lib.rsdsfm_noise_strength(ctypes.c_int64(5000), ctypes.c_int64(16), ctypes.c_int32(256), ctypes.c_int32(0), ctypes.c_int64(0)) == ERR_INVALID


def test_the_header_names_its_definition_and_its_symbols():
    assert "tests/noise_spec_numpy.py" in HEADER_TEXT and '#include "rsdsfm_denoise.h"' in HEADER_TEXT
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER_TEXT), name
    assert "choices, not measurements" in HEADER_TEXT and "NOT here" in HEADER_TEXT and "main.cc:380-523" in HEADER_TEXT
    for other in ("rsdsfm_denoise.h", "rsdsfm_denoise_spatial.h"):  # nothing new is declared in the existing headers
        txt = open(os.path.join(ROOT, "include", other)).read()
        assert not [n for n in NEW_SYMBOLS if re.search(r"\bint\s+%s\s*\(" % n, txt)] and "built since" in txt


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_symbols_are_exported_by_both_builds(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.noise_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    assert NEW_SYMBOLS <= set(rsdsfm.declared_symbols()) and not NEW_SYMBOLS & (set(rsdsfm.denoise_declared_symbols()) | set(rsdsfm.denoise_spatial_declared_symbols()))
    for name in ("noise_level_dev", "noise_level", "denoise_accumulate_auto_dev", "denoise_accumulate_auto", "denoise_spatial_auto_dev", "denoise_spatial_auto",
                 "denoise_auto_frame_dev", "denoise_auto_video_dev"):
        assert callable(getattr(rsdsfm.Solver, name))
    d = rsdsfm.noise_default_params()
    assert (d["quantile_q8"], d["scale"], d["min_samples"]) == (spec.QUANTILE_DEFAULT, spec.SCALE_DEFAULT, spec.MIN_SAMPLES_DEFAULT)
    assert ctypes.sizeof(rsdsfm.NoiseParams) == 40 and rsdsfm.NOISE_BINS == spec.BINS
    p = rsdsfm.NoiseParams()
    assert lib.rsdsfm_noise_params_init(ctypes.byref(p)) == 0 and p.struct_bytes == 40 and p.reserved0 == 0 and list(p.reserved) == [0, 0, 0, 0]
    assert ctypes.sizeof(rsdsfm.DenoiseParams) == 48 and ctypes.sizeof(rsdsfm.DenoiseSpatialParams) == 32  # the existing structs are as they were


def test_launch_counts_and_host_errors(rsdsfm):
    assert rsdsfm.noise_level_launches() == 2
    for r, c_ in ((2, 2), (37, 67), (720, 1280), (16384, 16384)):
        for n in (1, 2, 5, 15):
            assert rsdsfm.denoise_auto_frame_launches(r, c_, n) == rsdsfm.denoise_launches(r, c_, n) + 2
            assert rsdsfm.denoise_auto_frame_launches(r, c_, n, True) == rsdsfm.denoise_launches(r, c_, n) + 3
        for n in (0, -1, 16):
            with pytest.raises(rsdsfm.RsdsfmError):
                rsdsfm.denoise_auto_frame_launches(r, c_, n)
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.denoise_auto_frame_launches(r, c_, 2)
    lib = rsdsfm.load_library()
    i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert lib.rsdsfm_noise_params_init(None) == ERR_INVALID
    # no context: refused before anything is read
    assert lib.rsdsfm_noise_level_dev(None, None, None, i32(3), i32(8), i32(8), i32(0), None, None) == ERR_INVALID
    assert lib.rsdsfm_denoise_accumulate_auto_dev(None, None, None, None, None, i32(3), i32(8), i32(8), None, i64(0), i32(0), i32(0), None, i32(0), i64(0), None, i32(1), i32(1),
                                                  None, None, None, None) == ERR_INVALID
    assert lib.rsdsfm_denoise_spatial_auto_dev(None, None, None, None, i32(3), i32(8), i32(8), i32(0), None, i32(0), i64(0), i32(0), i32(0), None, None, None) == ERR_INVALID
    assert lib.rsdsfm_denoise_auto_frame_dev(None, None, i32(3), None, None, None, f64(1), f64(1), f64(0), f64(0), i32(8), i32(8), 0, 0, i32(0), i32(1), None, None, None, None,
                                             None, None, None, None, None, None, None, None) == ERR_INVALID
    assert lib.rsdsfm_denoise_auto_video_dev(None, None, i32(1), i32(8), i32(8), i32(3), f64(1), f64(1), f64(0), f64(0), None, None, None, None, None, None, None, None, 0, 0,
                                             i32(0), None, None, None, None, None, None, None, None, None, None) == ERR_INVALID
