"""Inputs of the temporal noise curve's tests (tests/test_noise_temporal_cpu.py, tests/test_gpu_noise_temporal.py) and of its golden fixture
(tests/golden/make_golden_noise_temporal.py): pairs for the histogram alone at the shapes where its kernel can go wrong (a tile is 16 rows x 64
columns), the scenes of the estimator's quality tests -- denoise_cases' noisy shift clip and the plate's mover on it -- and the measurements on
them."""
import numpy as np

import denoise_cases as dcases
import noise_curve_spec_numpy as cspec
import noise_spec_numpy as nspec
import noise_temporal_spec_numpy as spec
import plate_cases as pcases
import retime_cases as rcases

# no sample; one sample; exactly one tile; four workgroups with windows that straddle every tile edge; more tiles, cols % 4 = 2
PAIR_SHAPES = [(2, 2), (3, 3), (16, 64), (17, 65), (33, 130)]
# full: both masks full; holes: a few unset pixels in either mask, random non-zero bytes elsewhere; saturated: a few bytes of 0 and 255 in R and
# in L; empty: the layer's mask is empty
PAIR_KINDS = ["full", "holes", "saturated", "empty"]


def pair(rows, cols, channels, kind, seed=0, amp=3):
    """(ref, ref_mask, layer, layer_mask): the reference's levels cross every band along the columns; the layer is the reference within +-amp;
    random bytes under empty mask bytes"""
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed + 97 * PAIR_KINDS.index(kind) + 3)
    shape = (rows, cols, channels)
    x = np.arange(cols)
    base = (6 + (243 * x) // max(cols - 1, 1))[None, :, None] + np.zeros(shape, dtype=np.int64)
    ref = np.clip(base + rng.integers(-5, 6, size=shape), 1, 254)
    layer = np.clip(ref + rng.integers(-amp, amp + 1, size=shape), 1, 254)
    rmask, lmask = rng.integers(1, 256, size=(rows, cols)), rng.integers(1, 256, size=(rows, cols))
    if kind == "holes":
        rmask[rng.random((rows, cols)) < 0.02] = 0
        lmask[rng.random((rows, cols)) < 0.02] = 0
        for a, m in ((ref, rmask), (layer, lmask)):  # what lies under an unset pixel never shows
            a[m == 0] = rng.integers(0, 256, size=a[m == 0].shape)
    if kind == "saturated":
        for a in (ref, layer):
            hit = rng.random(shape) < 0.01
            a[hit] = rng.choice([0, 255], size=int(hit.sum()))
    if kind == "empty":
        lmask[:] = 0
    u8 = lambda a: np.ascontiguousarray(a.astype(np.uint8))
    ref, layer = u8(ref), u8(layer)
    return (ref[..., 0], u8(rmask), layer[..., 0], u8(lmask)) if channels == 1 else (ref, u8(rmask), layer, u8(lmask))


def pair_cases(shapes=PAIR_SHAPES):
    """every shape x channels x kind -> list of dicts, names unique"""
    out, k = [], 0
    for rows, cols in shapes:
        for channels in (1, 3):
            for kind in PAIR_KINDS:
                ref, rmask, layer, lmask = pair(rows, cols, channels, kind, seed=k)
                out.append(dict(name="%dx%dx%d-%s" % (rows, cols, channels, kind), ref=ref, rmask=rmask, layer=layer, lmask=lmask, kind=kind))
                k += 1
    assert len({c["name"] for c in out}) == len(out)
    return out


def golden_cases():
    """the pairs of (3, 3) and (17, 65), every kind, gray and BGR"""
    return pair_cases([(3, 3), (17, 65)])


def run_spec(case):
    return spec.pair_histogram(case["ref"], case["rmask"], case["layer"], case["lmask"])


# ---------------------------------------------------------------------------------------------------
# the estimator on the noisy shift clip
# ---------------------------------------------------------------------------------------------------
AMPS = (2, 6, 12, 20)
SEEDS = (0, 1, 2, 3)


def sigma_true(a):
    """of uniform integer noise in [-a, a]"""
    return float(np.sqrt(((2 * a + 1) ** 2 - 1) / 12.0))


def shift_measure(channels, a, seed):
    """the shift clip's middle frame at radius 2 under noise +-a -> dict(case, run (denoise_cases.run_spec's), temporal, spatial (the two
    measurements' dict(hist, curve)))"""
    case = dcases.shift_clip(seed, channels, noise=a)
    run = dcases.run_spec(case)
    ref, rmask, _ = run["ref"]
    return dict(case=case, run=run, temporal=spec.noise_temporal(ref, rmask, run["layers"], list(run["records"])), spatial=cspec.noise_curve(ref, rmask))


def sigma_hat(curve):
    return int(curve[8, 2]) / 256.0


def strength_of(curve):
    """row 8's strength at the defaults: noise_spec_numpy.noise_strength"""
    return nspec.noise_strength(int(curve[8, 0]), int(curve[8, 1]))


def error_ratio(case, image):
    """mean absolute error against the clean frame over the columns every source sees, output / noisy own frame"""
    q = case["q"]
    cols_ok = dcases.shift_seen_by_all(case)
    clean = case["clean"][q].astype(np.int64)
    err = lambda img: np.abs(img.astype(np.int64) - clean)[:, cols_ok].mean()
    return err(image) / err(case["frames"][q])


def denoise_ratios(m):
    """shift_measure's dict -> (error ratio at the temporal curve's strengths, at the fixed default 12)"""
    run = m["run"]
    ref, rmask, _ = run["ref"]
    lut = cspec.strengths(m["temporal"]["curve"])
    out = cspec.denoise(ref, rmask, run["layers"], lut, list(run["records"]))
    return error_ratio(m["case"], out["image"]), error_ratio(m["case"], run["image"])


# ---------------------------------------------------------------------------------------------------
# the plate's mover on the shift texture
# ---------------------------------------------------------------------------------------------------
MOVER_NOISE = 2


def mover_measure(seed):
    """plate_cases.mover_scene's geometry at noise +-2 and the given seed: a block of 255 that sits four columns further in every frame of frame
    q's camera.  -> dict(temporal, spatial: the mean absolute error against the clean texture under the NEIGHBOURS' footprints in frame q, where
    a ghost would show; h_temporal, h_spatial: row 8's strengths)"""
    case = dcases.shift_clip(seed=seed, channels=3, q=2, radius=2, noise=MOVER_NOISE, name="mover-%d" % seed, nframes=5, cols=pcases.MOVER_COLS)
    rows = case["depths"][0].shape[0]
    frames, prints = [], np.zeros((5, rows, pcases.MOVER_COLS), dtype=bool)
    r0, r1 = pcases.MOVER_ROWS
    for n, frame in enumerate(case["frames"]):
        x = pcases.MOVER_TARGET_COLUMNS[n] - rcases.SHIFT * (n - case["q"])
        frame = frame.copy()
        frame[r0:r1, x:x + pcases.MOVER_WIDTH] = 255
        frames.append(frame)
        prints[n, r0:r1, pcases.MOVER_TARGET_COLUMNS[n]:pcases.MOVER_TARGET_COLUMNS[n] + pcases.MOVER_WIDTH] = True
    case = dict(case, frames=frames, gain_mode=1)
    run = dcases.run_spec(case)
    ref, rmask, _ = run["ref"]
    ghost = prints[[0, 1, 3, 4]].any(axis=0) & ~prints[2]
    clean = case["clean"][2].astype(np.int64)
    out = {}
    for name, curve in (("temporal", spec.noise_temporal(ref, rmask, run["layers"], list(run["records"]), gain_mode=1)["curve"]), ("spatial", cspec.noise_curve(ref, rmask)["curve"])):
        img = cspec.denoise(ref, rmask, run["layers"], cspec.strengths(curve), list(run["records"]), gain_mode=1)["image"]
        out[name] = float(np.abs(img.astype(np.int64) - clean)[ghost].mean())
        out["h_" + name] = strength_of(curve)
    return out
