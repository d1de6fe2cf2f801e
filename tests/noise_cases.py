"""Inputs of the noise level's tests (tests/test_noise_cpu.py, tests/test_gpu_noise.py) and of its golden fixture
(tests/golden/make_golden_noise.py): frames for the primitive at the shapes where its kernel can go wrong (a tile is 16 rows x 64 columns, a
thread owns 4 consecutive pixels, a sample needs its whole 3 x 3 window), the quality scene at any noise amplitude, and the static clip that shows
what the estimated strength is for."""
import numpy as np

import noise_spec_numpy as spec

# no sample (2 rows, 2 columns); one sample; two; a byte tail; exactly the tile, one over and two over in both directions (the halo's far side);
# several tiles with rows that start on other bytes of a dword (cols % 4 = 2, 3)
SHAPES = [(2, 2), (2, 9), (3, 3), (3, 4), (4, 7), (16, 64), (17, 65), (18, 66), (33, 130), (35, 67)]
KINDS = ["noisy", "holes", "clipped", "flat", "checker"]
QUANTILES = [0, 1, 128, 256]  # 0: the default
GOLDEN_SHAPES = [(2, 9), (3, 3), (4, 7), (18, 66)]


def frame(rows, cols, channels, kind, seed=0):
    """(image, mask).  noisy: a smooth ramp under uniform noise whose amplitude changes with the seed, the mask all set with arbitrary non-zero
    bytes; holes: the same under a mask with about 15 % of its bytes 0; clipped: the same with about 4 % of the image bytes 0 or 255; flat: 128
    everywhere, every sample in bin 0 -- the contention path; checker: 1 / 254 alternating, |r| = 16 * 253 / 2 = 2024, the clamp bin"""
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed + 101 * KINDS.index(kind) + 7)
    shape = (rows, cols, channels)
    y, x = np.mgrid[0:rows, 0:cols]
    amp = [1, 3, 8, 25][seed % 4]
    base = (60 + 2 * x + 3 * y + 0 * x * y)[..., None] % 180 + 30 + 7 * np.arange(channels)
    image = np.clip(base + rng.integers(-amp, amp + 1, size=shape), 1, 254)
    mask = rng.integers(1, 256, size=(rows, cols))
    if kind == "holes":
        mask = np.where(rng.random((rows, cols)) < 0.15, 0, mask)
        image = np.where((mask == 0)[..., None], rng.integers(0, 256, size=shape), image)  # random bytes under unset mask bytes
    elif kind == "clipped":
        pick = rng.random(shape)
        image = np.where(pick < 0.02, 0, np.where(pick < 0.04, 255, image))
    elif kind == "flat":
        image = np.full(shape, 128)
    elif kind == "checker":
        image = np.where(((x + y) % 2 == 0)[..., None], 1, 254) + np.zeros(shape, dtype=np.int64)
    image = image.astype(np.uint8)
    return (image[..., 0] if channels == 1 else image), mask.astype(np.uint8)


def primitive_cases(shapes=SHAPES):
    """every shape x channels x kind, the quantile and the seed cycling -> list of dicts, names unique.  Asserts what the set must cover: a
    case without a sample, the clamp bin hit, a sample dropped for clipping, a candidate dropped by the mask"""
    out, k = [], 0
    for rows, cols in shapes:
        for channels in (1, 3):
            for kind in KINDS:
                image, mask = frame(rows, cols, channels, kind, seed=k)
                out.append(dict(name="%dx%dx%d-%s" % (rows, cols, channels, kind), image=image, mask=mask, quantile_q8=QUANTILES[k % len(QUANTILES)], kind=kind))
                k += 1
    assert len({c["name"] for c in out}) == len(out)
    if shapes is SHAPES:
        covered = dict(empty=False, clamp=False, clipped=False, masked=False)
        for c in out:
            r = run_spec(c)
            _, sample = spec.responses(c["image"], c["mask"])
            full = spec.responses(c["image"], np.ones_like(c["mask"]))[1]
            covered["empty"] |= int(r["record"][0]) == 0
            covered["clamp"] |= int(r["hist"][spec.BINS - 1]) > 0
            covered["clipped"] |= c["kind"] == "clipped" and bool((~sample).any())
            covered["masked"] |= c["kind"] == "holes" and int(full.sum()) > int(sample.sum())
        assert all(covered.values()), covered
    return out


def golden_cases():
    """every kind, both channel counts and every quantile on the small shapes"""
    every = primitive_cases(GOLDEN_SHAPES)
    return [every[i] for i in (0, 3, 6, 11, 14, 17, 22, 25, 28, 30, 32, 39)]


def run_spec(case, **over):
    c = dict(case, **over)
    return spec.noise_level(c["image"], c["mask"], c["quantile_q8"])


# ---------------------------------------------------------------------------------------------------
# the quality scene (tests/denoise_spatial_cases.py's, at any amplitude) and the static clip
# ---------------------------------------------------------------------------------------------------
QUALITY_ROWS, QUALITY_COLS, QUALITY_SEEDS = 96, 130, 8
AMPLITUDES = [2, 4, 6, 9, 12, 20]
CLIP_FRAMES = 5


def quality_clean(channels):
    """(rows, cols, channels) int64: a smooth wave on a checkerboard of 16 x 16 with a step of 40"""
    y, x = np.mgrid[0:QUALITY_ROWS, 0:QUALITY_COLS]
    return np.stack([np.clip(np.rint(110 + 60 * np.sin(x / 9 + c) * np.cos(y / 7) + 40 * ((x // 16 + y // 16) % 2)), 0, 255) for c in range(channels)], axis=-1).astype(np.int64)


def quality_clip(channels, seed, a):
    """-> (clean (rows, cols, channels) int64, five noisy frames uint8 (rows, cols[, 3])): the static scene under uniform integer noise in
    [-a, a], independent per frame"""
    clean = quality_clean(channels)
    rng = np.random.default_rng(1000 * a + seed)
    frames = [np.clip(clean + rng.integers(-a, a + 1, size=clean.shape), 0, 255).astype(np.uint8) for _ in range(CLIP_FRAMES)]
    return clean, [f[..., 0] if channels == 1 else f for f in frames]


def sigma_true(a):
    """the standard deviation of the uniform integers in [-a, a]"""
    return (a * (a + 1) / 3.0) ** 0.5
