"""Inputs of the spatial top-up's tests (tests/test_denoise_spatial_cpu.py, tests/test_gpu_denoise_spatial.py) and of its golden fixture
(tests/golden/make_golden_denoise_spatial.py): frames for the primitive at the shapes where its kernel can go wrong (a tile is 16 rows x 64
columns, a thread owns 4 consecutive pixels, the halo is search + 1), the quality scene, and the mover scene that shows what the stage is for."""
import numpy as np

import denoise_spatial_spec_numpy as spec
import denoise_spec_numpy as temporal

# one word; a byte tail; one under, exactly one and one over the tile in both directions; several tiles with rows that start on other bytes of a
# dword (cols % 4 = 2, 3)
SHAPES = [(2, 2), (2, 9), (15, 63), (16, 64), (17, 65), (33, 130), (5, 131)]
SEARCHES = [1, 2, 3]
# strength and target at 1, at 255 and at the defaults (0: the call's default)
PARAMS = [(0, 0), (1, 255), (255, 1), (12, 255), (255, 80), (1, 1), (40, 120)]
GOLDEN_SHAPES = [(2, 2), (2, 9), (7, 11), (12, 19)]


def frame(rows, cols, channels, seed=0, set_fraction=0.8):
    """(image, mask, weight): blocks of 4 x 6 pixels of one colour under noise whose amplitude changes from block to block (0, +-2, +-8, random
    bytes), so that the patch errors -- and the weights -- take every value from 0 to 16; a mask that is set on about 80 % of the pixels with
    arbitrary non-zero bytes, random image bytes under unset mask bytes too; weights over the whole byte range, a quarter of them 0, 16 or 80"""
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed + 3)
    shape = (rows, cols, channels)
    up = lambda a: a.repeat(4, axis=0).repeat(6, axis=1)[:rows, :cols]
    base = up(rng.integers(20, 236, size=((rows + 3) // 4, (cols + 5) // 6, channels)))
    kind = up(rng.integers(0, 4, size=((rows + 3) // 4, (cols + 5) // 6, 1)))
    amp = np.array([0, 2, 8, 0])[kind]
    noisy = np.clip(base + np.rint((2 * rng.random(shape) - 1) * amp).astype(np.int64), 0, 255)
    image = np.where(kind == 3, rng.integers(0, 256, size=shape), noisy).astype(np.uint8)
    mask = np.where(rng.random((rows, cols)) < set_fraction, rng.integers(1, 256, size=(rows, cols)), 0).astype(np.uint8)
    weight = rng.integers(0, 256, size=(rows, cols))
    pick = rng.random((rows, cols))
    weight = np.where(pick < 0.08, 0, np.where(pick < 0.16, 16, np.where(pick < 0.25, 80, np.where(pick < 0.6, weight // 4, weight)))).astype(np.uint8)
    return (image[..., 0] if channels == 1 else image), mask, weight


def primitive_cases(shapes=SHAPES):
    """every shape x channels x search, the parameters and the presence of the weight plane cycling -> list of dicts, names unique"""
    out, k = [], 0
    for rows, cols in shapes:
        for channels in (1, 3):
            for search in SEARCHES:
                image, mask, weight = frame(rows, cols, channels, seed=search)
                strength, target = PARAMS[k % len(PARAMS)]
                out.append(dict(name="%dx%dx%d-s%d" % (rows, cols, channels, search), image=image, mask=mask, weight=weight if k % 3 else None, strength=strength, target=target,
                                search=search))
                k += 1
    assert len({c["name"] for c in out}) == len(out)
    return out


def golden_cases():
    """nine of the small cases: every shape, both channel counts, every search, with and without the weight plane"""
    every = primitive_cases(GOLDEN_SHAPES)
    return [every[i] for i in (1, 5, 6, 10, 14, 15, 19, 21, 23)]


def run_spec(case, **over):
    c = dict(case, **over)
    return spec.denoise_spatial(c["image"], c["mask"], c["weight"], c["strength"] or spec.STRENGTH_DEFAULT, c["target"] or spec.TARGET_DEFAULT,
                                c["search"] or spec.SEARCH_DEFAULT)


# ---------------------------------------------------------------------------------------------------
# the quality scene
# ---------------------------------------------------------------------------------------------------
QUALITY_ROWS, QUALITY_COLS, QUALITY_NOISE, QUALITY_SEEDS = 96, 130, 6, 8


def quality_scene(channels, seed):
    """-> (clean (rows, cols, channels) int64, noisy uint8 (rows, cols[, 3])): a smooth wave on a checkerboard of 16 x 16 with a step of 40, under
    uniform integer noise in [-6, 6]"""
    y, x = np.mgrid[0:QUALITY_ROWS, 0:QUALITY_COLS]
    clean = np.stack([np.clip(np.rint(110 + 60 * np.sin(x / 9 + c) * np.cos(y / 7) + 40 * ((x // 16 + y // 16) % 2)), 0, 255) for c in range(channels)], axis=-1).astype(np.int64)
    noisy = np.clip(clean + np.random.default_rng(seed).integers(-QUALITY_NOISE, QUALITY_NOISE + 1, size=clean.shape), 0, 255).astype(np.uint8)
    return clean, (noisy[..., 0] if channels == 1 else noisy)


# ---------------------------------------------------------------------------------------------------
# the mover scene
# ---------------------------------------------------------------------------------------------------
MOVER = (10, 6, 12, 14, 9, 1)  # (y0, x0, h, w, dx, dy): it moves by more than half its width per frame
MOVER_FRAMES, MOVER_ROWS, MOVER_COLS, MOVER_NOISE, MOVER_Q = 5, 40, 72, 6, 2


def mover_scene(synth):
    """synth.render_sequence's static scene (no camera motion: every frame is registered as it is) with a block moving through it, five frames
    under sensor noise of +-6, the middle frame through the temporal definition with its four neighbours as layers
    -> dict(clean, noisy: the middle frame without and with noise, temporal: the definition's dict, own_only: weight == 16)"""
    K = (60.0, 60.0, MOVER_COLS / 2.0, MOVER_ROWS / 2.0)
    zero = np.zeros(3)
    kw = dict(seed=77, mover=MOVER)
    clean = synth.render_sequence(MOVER_FRAMES, MOVER_ROWS, MOVER_COLS, K, zero, zero, **kw)[0]
    noisy = synth.render_sequence(MOVER_FRAMES, MOVER_ROWS, MOVER_COLS, K, zero, zero, noise=MOVER_NOISE, **kw)[0]
    full = np.ones((MOVER_ROWS, MOVER_COLS), dtype=np.uint8)
    layers = [(noisy[n], full) for n in temporal.neighbour_order(MOVER_Q, MOVER_FRAMES, 2)[1:]]
    r = temporal.denoise(noisy[MOVER_Q], full, layers)
    return dict(clean=clean[MOVER_Q], noisy=noisy[MOVER_Q], temporal=r, own_only=r["weight"] == temporal.W, mask=full)
