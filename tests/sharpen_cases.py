"""Inputs of the sharpen stage's tests (tests/test_sharpen_cpu.py, tests/test_gpu_sharpen.py) and of its golden fixture
(tests/golden/make_golden_sharpen.py): the shapes, the kinds of frame, the parameter sets, and the quality scene."""
import numpy as np

import sharpen_spec_numpy as spec

# the smallest shapes at which the 16 x 64 tile, the halo of 2 across a tile border, the byte paths for cols % 4 != 0 and frames smaller than
# the halo can go wrong
SHAPES = [(2, 2), (2, 9), (3, 3), (4, 7), (5, 5), (16, 64), (17, 65), (18, 66), (20, 68), (33, 130), (35, 67)]
# noisy: a smooth field under noise, full mask; holes: the same with a third of the mask unset; clipped: bytes 0 and 255 in blocks; flat: one
# value; checker: 0 / 255 alternating, the largest detail; ramp: affine in (x, y); isolated: single set pixels among unset; step: step edges
KINDS = ["noisy", "holes", "clipped", "flat", "checker", "ramp", "isolated", "step"]
# (amount_q4, coring_q4, overshoot), cycling
PARAMS = [(16, 8, 0), (64, 0, 255), (1, 64, 0), (0, 8, 0), (32, 8, 8)]
GOLDEN_SHAPES = [(3, 3), (4, 7), (18, 66)]


def frame(rows, cols, channels, kind, seed=0):
    """(image, mask) uint8"""
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed + 101 * KINDS.index(kind) + 3)
    shape = (rows, cols, channels)
    y, x = np.mgrid[0:rows, 0:cols]
    mask = rng.integers(1, 256, size=(rows, cols))
    if kind in ("noisy", "holes"):
        base = 128 + 60 * np.sin(x / 5.0 + seed) * np.cos(y / 4.0)
        image = np.rint(base)[..., None] + rng.integers(-12, 13, size=shape) + 9 * np.arange(channels)
        if kind == "holes":
            mask[rng.random((rows, cols)) < 0.33] = 0
    elif kind == "clipped":
        image = np.where(((x // 3 + y // 2) % 2)[..., None] == 0, 0, 255) + np.zeros(shape, dtype=np.int64)
        image = np.where(rng.random(shape) < 0.2, rng.integers(0, 256, size=shape), image)
    elif kind == "flat":
        image = np.full(shape, 37 + 50 * (seed % 4), dtype=np.int64)
        mask[rng.random((rows, cols)) < 0.1] = 0
    elif kind == "checker":
        image = (255 * ((x + y) % 2))[..., None] + np.zeros(shape, dtype=np.int64)
    elif kind == "ramp":
        image = (3 * x + y)[..., None] + 5 * np.arange(channels) + np.zeros(shape, dtype=np.int64)
    elif kind == "isolated":
        image = rng.integers(0, 256, size=shape)
        mask = np.where((x % 3 == 0) & (y % 3 == 0), mask, 0)  # pixels 3 apart: two of a 5 x 5 block are set, none of a 3 x 3 but the centre
        mask[rng.random((rows, cols)) < 0.05] = 200
    else:
        image = np.where((x >= cols // 2)[..., None], 200, 40) + np.where((y >= rows // 2)[..., None], 30, 0) + rng.integers(-2, 3, size=shape)
    image = np.clip(image, 0, 255).astype(np.uint8)
    return (image[..., 0] if channels == 1 else image), mask.astype(np.uint8)


def primitive_cases(shapes=SHAPES):
    """every shape x channels x kind, the parameter set, the strength and the seed cycling -> list of dicts, names unique.  Asserts what the set
    must cover: every counter non-zero in some case, every parameter set met by every kind, and a set pixel with K < 121 (a hole in its block)"""
    out, k = [], 0
    for rows, cols in shapes:
        for channels in (1, 3):
            for kind in KINDS:
                image, mask = frame(rows, cols, channels, kind, seed=k)
                amount, coring, overshoot = PARAMS[k % len(PARAMS)]
                out.append(dict(name="%dx%dx%d-%s" % (rows, cols, channels, kind), image=image, mask=mask, amount_q4=amount, coring_q4=coring, overshoot=overshoot,
                                strength=(12, 1, 255, 30)[k % 4], kind=kind))
                k += 1
    assert len({c["name"] for c in out}) == len(out)
    if shapes is SHAPES:
        total = np.zeros(4, dtype=np.int64)
        met = set()
        small_K = False
        for c in out:
            total += np.array(run_spec(c)["counts"])
            met.add((c["kind"], (c["amount_q4"], c["coring_q4"], c["overshoot"])))
            _, K = spec.blur_sums(c["image"], c["mask"])
            small_K |= bool(((c["mask"] != 0) & (K < 121)).any())
        assert (total > 0).all() and small_K, (total, small_K)
        assert len(met) == len(KINDS) * len(PARAMS), len(met)
    return out


def run_spec(case, lut=None):
    return spec.sharpen(case["image"], case["mask"], case["amount_q4"], case["coring_q4"], case["overshoot"], case["strength"], lut)


def golden_cases():
    """a few tiny cases: every kind once on (18, 66), alternating gray and BGR, and every parameter set once on (4, 7) or (3, 3)"""
    every = primitive_cases(GOLDEN_SHAPES)
    big = [c for c in every if c["image"].shape[:2] == (18, 66)]
    small = [c for c in every if c["image"].shape[:2] != (18, 66)]
    picked = [[c for c in big if c["kind"] == kind][i % 2] for i, kind in enumerate(KINDS)]
    for p in PARAMS:
        picked.append([c for c in small if (c["amount_q4"], c["coring_q4"], c["overshoot"]) == p][0])
    return picked


def golden_curve_case():
    """(image, mask, lut): a BGR ramp through every level under the table of noise_curve_cases' rising curve"""
    import noise_curve_cases as ccases
    import noise_curve_spec_numpy as cspec

    image, mask = ccases.ramp_reference(17, 65, 3, seed=1)
    return image, mask, cspec.strengths(ccases.RISING)


# ---------------------------------------------------------------------------------------------------
# the quality scene: a flat third and an edge texture, blurred by a 3 x 3 binomial "sensor", under uniform noise
# ---------------------------------------------------------------------------------------------------
QUALITY_ROWS, QUALITY_COLS, QUALITY_SEEDS = 96, 130, 8
QUALITY_AMPS = (2, 6, 12)
QUALITY_FLAT_COLS = QUALITY_COLS // 3


def quality_clean():
    """(rows, cols) int64: the left third flat at 120, the rest bars and blocks of 70 / 180, 5 and 7 pixels wide"""
    y, x = np.mgrid[0:QUALITY_ROWS, 0:QUALITY_COLS]
    texture = np.where(((x // 5) + (y // 7)) % 2 == 0, 70, 180)
    return np.where(x < QUALITY_FLAT_COLS, 120, texture).astype(np.int64)


def sensor_blur(clean):
    """the 3 x 3 binomial [1, 2, 1]^2 / 16 with replicated borders, rounded half up"""
    p = np.pad(clean, 1, mode="edge")
    rows, cols = clean.shape
    acc = np.zeros_like(clean)
    for dy, wy in enumerate((1, 2, 1)):
        for dx, wx in enumerate((1, 2, 1)):
            acc += wy * wx * p[dy:dy + rows, dx:dx + cols]
    return (acc + 8) // 16


def quality_frame(seed, a):
    """-> (clean int64, observed uint8): the blurred clean frame under uniform integer noise in [-a, a]"""
    clean = quality_clean()
    rng = np.random.default_rng(1000 * a + seed)
    return clean, np.clip(sensor_blur(clean) + rng.integers(-a, a + 1, size=clean.shape), 0, 255).astype(np.uint8)


def quality_regions():
    """(textured, flat) boolean masks, each 3 pixels inside its region and the frame"""
    y, x = np.mgrid[0:QUALITY_ROWS, 0:QUALITY_COLS]
    inside = (y >= 3) & (y < QUALITY_ROWS - 3)
    return inside & (x >= QUALITY_FLAT_COLS + 3) & (x < QUALITY_COLS - 3), inside & (x >= 3) & (x < QUALITY_FLAT_COLS - 3)
