"""Inputs of the noise curve's tests (tests/test_noise_curve_cpu.py, tests/test_gpu_noise_curve.py) and of its golden fixture
(tests/golden/make_golden_noise_curve.py): noise_cases' shapes and kinds, three kinds of its own that exercise the bands, hand-made curves for
the consumers, and the ramp scene whose noise grows with brightness."""
import numpy as np

import noise_cases as ncases
import noise_curve_spec_numpy as spec

SHAPES = ncases.SHAPES
# ramp: levels crossing all eight bands inside one tile; two_level: only bands 1 and 6 populated (the fill and its ties); band_edge: levels
# 31 / 32 and 223 / 224 alternating (the band of L against the band of the centre byte)
KINDS = ncases.KINDS + ["ramp", "two_level", "band_edge"]
QUANTILES = ncases.QUANTILES
GOLDEN_SHAPES = [(3, 4), (4, 7), (18, 66)]
# the cases are small: the defaults (1024 and 256 samples) are more than some of them have
MIN_SAMPLES, BAND_MIN_SAMPLES = 64, 16


def frame(rows, cols, channels, kind, seed=0):
    """(image, mask): noise_cases.frame for its kinds.  ramp: 8 .. 247 across at most 64 columns (so every band lies inside one tile) under
    noise that grows with the level; two_level: the left half about 48, the right half about 208; band_edge: rows of 31 / 32 and of 223 / 224 in
    a checkerboard, so that a centre byte of 31 (band 0) has L = 32 (band 1) about as often as not"""
    if kind in ncases.KINDS:
        return ncases.frame(rows, cols, channels, kind, seed)
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed + 101 * KINDS.index(kind) + 7)
    shape = (rows, cols, channels)
    y, x = np.mgrid[0:rows, 0:cols]
    if kind == "ramp":
        base = (8 + (239 * (x % 64)) // max(min(cols, 64) - 1, 1))[..., None] + np.zeros(shape, dtype=np.int64)
        amp = 1 + base // 40
        image = np.clip(base + np.rint((2 * rng.random(shape) - 1) * amp).astype(np.int64), 1, 254)
    elif kind == "two_level":
        base = np.where(x < cols // 2, 48, 208)[..., None] + np.zeros(shape, dtype=np.int64)
        image = base + rng.integers(-3, 4, size=shape) * np.where(base > 128, 3, 1)
    else:
        lo = np.where(y < rows // 2, 31, 223)[..., None] + np.zeros(shape, dtype=np.int64)
        image = lo + ((x + y) % 2)[..., None] + (rng.random(shape) < 0.1)  # a few bytes one up: |r| is not one value
    mask = rng.integers(1, 256, size=(rows, cols))
    if kind == "two_level":
        mask[:, cols // 2] = 0  # no window spans both halves: no sample at a level between them
    image = image.astype(np.uint8)
    return (image[..., 0] if channels == 1 else image), mask.astype(np.uint8)


def primitive_cases(shapes=SHAPES):
    """every shape x channels x kind, the quantile and the seed cycling -> list of dicts, names unique.  Asserts what the set must cover: all
    eight bands populated in one case, exactly bands 1 and 6 in another, and a sample whose band differs from its centre byte's"""
    out, k = [], 0
    for rows, cols in shapes:
        for channels in (1, 3):
            for kind in KINDS:
                image, mask = frame(rows, cols, channels, kind, seed=k)
                out.append(dict(name="%dx%dx%d-%s" % (rows, cols, channels, kind), image=image, mask=mask, quantile_q8=QUANTILES[k % len(QUANTILES)], kind=kind))
                k += 1
    assert len({c["name"] for c in out}) == len(out)
    if shapes is SHAPES:
        covered = dict(all_bands=False, two_bands=False, edge=False)
        for c in out:
            n = spec.histogram(c["image"], c["mask"]).sum(axis=1)
            covered["all_bands"] |= c["kind"] == "ramp" and bool((n > 0).all())
            covered["two_bands"] |= c["kind"] == "two_level" and [b for b in range(8) if n[b]] == [1, 6]
            if c["kind"] == "band_edge" and c["image"].shape[0] > 2 and c["image"].shape[1] > 2:
                L = spec.levels(c["image"])[..., 0]
                centre = spec.noise._planes(c["image"])[1:-1, 1:-1, 0].astype(np.int64)
                covered["edge"] |= bool(((L >> 5) != (centre >> 5)).any())
        assert all(covered.values()), covered
    return out


def golden_cases():
    """a few tiny cases: the three kinds of this file on (18, 66), gray and BGR, and every kind once on (4, 7) or (3, 4)"""
    every = primitive_cases(GOLDEN_SHAPES)
    new = [c for c in every if c["kind"] in KINDS[-3:] and c["image"].shape[:2] == (18, 66)]
    small = [c for c in every if c["image"].shape[:2] != (18, 66)]
    return new + [[c for c in small if c["kind"] == kind][i % 4] for i, kind in enumerate(KINDS)]


def run_spec(case):
    return spec.noise_curve(case["image"], case["mask"], case["quantile_q8"])


# ---------------------------------------------------------------------------------------------------
# hand-made curves for the consumers
# ---------------------------------------------------------------------------------------------------
def record(n, m):
    return [n, m, (256000 * m + 2023) // 4047, 0]


def curve(ns, ms, n8, m8):
    """(9, 4) uint64 from eight (n, m) and row 8's"""
    return np.array([record(n, m) for n, m in zip(ns, ms)] + [record(n8, m8)], dtype=np.uint64)


def flat_curve(n, m):
    return curve([n] * 8, [m] * 8, 8 * n, m)


RISING = curve([300] * 8, [3, 6, 10, 15, 22, 30, 41, 60], 2400, 20)          # every band valid, m rising with the level
GAPS = curve([300, 0, 5, 300, 0, 0, 300, 2], [40, 999, 999, 4, 999, 999, 90, 999], 907, 30)  # invalid bands: the fill and its ties
NO_BAND = curve([3] * 8, [500] * 8, 2000, 25)                                  # no band valid: row 8's m everywhere
TOO_FEW = curve([300] * 8, [3, 6, 10, 15, 22, 30, 41, 60], 50, 20)             # row 8 below min_samples: the fallback
# (curve, fallback, scale, min_samples, band_min_samples)
CURVES = [(RISING, 0, 0, 0, 0), (GAPS, 40, 24, 64, 16), (NO_BAND, 7, 0, 0, 0), (TOO_FEW, 33, 0, MIN_SAMPLES, BAND_MIN_SAMPLES), (RISING, 200, 255, 1, 1)]


def ramp_reference(rows, cols, channels, seed=0):
    """(image, mask): levels from 4 to 251 across the columns under a little noise, so that the consumers read the whole table; the mask is
    denoise_cases.reference's"""
    import denoise_cases as dcases

    _, mask = dcases.reference(rows, cols, channels, seed)
    rng = np.random.default_rng(rows * 31 + cols * 7 + channels + seed)
    x = np.arange(cols)
    base = (4 + (247 * x) // max(cols - 1, 1))[None, :, None] + np.zeros((rows, cols, channels), dtype=np.int64)
    image = np.clip(base + rng.integers(-4, 5, size=base.shape) + 5 * np.arange(channels), 0, 255).astype(np.uint8)
    return (image[..., 0] if channels == 1 else image), mask


# ---------------------------------------------------------------------------------------------------
# the quality scene: a static ramp whose noise grows with brightness
# ---------------------------------------------------------------------------------------------------
QUALITY_ROWS, QUALITY_COLS, QUALITY_SEEDS, QUALITY_FRAMES = 96, 130, 8, 5
QUALITY_AMPS = (2, 20)


def ramp_clean(channels):
    """(rows, cols, channels) int64: 20 .. 235 across the columns with a +-5 block texture"""
    y, x = np.mgrid[0:QUALITY_ROWS, 0:QUALITY_COLS]
    base = 20 + (215 * x) // (QUALITY_COLS - 1) + 5 * (2 * ((x // 8 + y // 8) % 2) - 1)
    return np.stack([base] * channels, axis=-1).astype(np.int64)


def amplitude(v, a0, a255):
    """the noise amplitude at the value v: a0 + ((a255 - a0) v + 127) // 255"""
    return a0 + ((a255 - a0) * v + 127) // 255


def ramp_clip(channels, seed, a0, a255):
    """-> (clean, five noisy frames uint8): uniform integer noise in [-a(v), a(v)], independent per frame"""
    clean = ramp_clean(channels)
    amp = amplitude(clean, a0, a255)
    rng = np.random.default_rng(100000 * a0 + 1000 * a255 + seed)
    frames = [np.clip(clean + rng.integers(-amp, amp + 1), 0, 255).astype(np.uint8) for _ in range(QUALITY_FRAMES)]
    return clean, [f[..., 0] if channels == 1 else f for f in frames]
