"""Inputs of the super-resolution's tests (tests/test_superres_cpu.py, tests/test_gpu_superres.py) and of its golden fixture
(tests/golden/make_golden_superres.py): sources for the render alone at the shapes where its kernel can go wrong (a lane owns 4 fine pixels
of a row), planes for the accumulate alone at the denoise's shapes, the aliased shift scene of the quality test, and small solved clips for
the frame and clip calls, built from the denoise's scenes (tests/denoise_cases.py, reused as they are)."""
import numpy as np

import denoise_cases as dcases
import shutter_cases as scases
import superres_spec_numpy as spec

TILE_ROWS, TILE_COLS = dcases.TILE_ROWS, dcases.TILE_COLS
ACC_SHAPES = dcases.ACC_SHAPES
ACC_LAYERS = dcases.ACC_LAYERS
records = dcases.records
impulse_positions = dcases.impulse_positions

# (source rows, source cols, scale): one word at every scale; fine rows of 14 columns (a tail); fine 18 x 66, across a tile both ways; scale 1
# with a tail; fine 24 x 66 and 20 x 68
RENDER_SHAPES = [(2, 2, 1), (2, 2, 2), (2, 2, 3), (2, 2, 4), (3, 7, 2), (9, 33, 2), (17, 65, 1), (8, 22, 3), (5, 17, 4)]


# ---------------------------------------------------------------------------------------------------
# sources for the render alone
# ---------------------------------------------------------------------------------------------------
def render_source(rows, cols, channels, kind="pose", seed=0):
    """one source: random bytes, a smooth depth, a rolling-shutter pose table that turns a little from scanline to scanline, and the pose (M, m)
    of the target camera.  kind: "identity" (constant depth, identity poses: the render is a pure upscale), "pose" (a non-identity pose, holes
    in the depth), "empty" (no valid depth)"""
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed + 3)
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    image = rng.integers(0, 256, size=shape, dtype=np.uint8)
    K = (1.5 * cols, 1.5 * cols, 0.5 * cols - 0.25, 0.5 * rows + 0.125)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    if kind == "identity":
        depth = np.full((rows, cols), 4.0)
        R, t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
        M, m = np.eye(3), np.zeros(3)
    else:
        depth = 4.0 + 0.5 * np.sin(0.7 * x + 0.3) * np.cos(0.5 * y) + 0.05 * rng.random((rows, cols))
        depth[rng.random((rows, cols)) < 0.15] = 0.0  # holes, filled by stage A
        depth[0, 0] = np.nan
        if not (depth > 0).any():
            depth[rows - 1, cols - 1] = 4.0
        import link_spec_numpy as link

        R = np.stack([link.rodrigues(np.array([0.0004, -0.0007, 0.0005]) * r).reshape(9) for r in range(rows)])
        t = np.stack([np.array([0.002, -0.001, 0.0005]) * r for r in range(rows)])
        M, m = link.rodrigues(np.array([0.004, -0.006, 0.01])), np.array([0.03, -0.02, 0.01])
        if kind == "empty":
            depth = np.where(rng.random((rows, cols)) < 0.5, 0.0, -1.0)
            depth[0, 0] = np.inf
    return dict(image=image, depth=depth, R=R, t=t, K=K, M=M, m=m)


# ---------------------------------------------------------------------------------------------------
# planes for the accumulate alone
# ---------------------------------------------------------------------------------------------------
def prox_plane(rows, cols, phase, rng):
    """shutter_cases.sample_mask's pattern of empty, full and mixed words with the set bytes drawn from 1 .. 16"""
    on = scases.sample_mask(rows, cols, phase, rng) != 0
    return (on * rng.integers(1, spec.PROX_MAX + 1, size=(rows, cols))).astype(np.uint8)


def reference(rows, cols, channels, seed=0):
    """(bil, near, prox): random bytes everywhere -- also where prox is 0 -- near within +-12 of bil"""
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed + 6)
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    bil = rng.integers(0, 256, size=shape, dtype=np.uint8)
    near = np.clip(bil.astype(np.int64) + rng.integers(-12, 13, size=shape), 0, 255).astype(np.uint8)
    return bil, near, prox_plane(rows, cols, 3 + seed, rng)


def layers(ref, rows, cols, channels, L, seed=0):
    """L layers (bil, near, prox): the bilinear planes are denoise_cases.layers' (the reference, the reference within +-3, within +-20, random, in
    patches, so that the patch weight takes every value), near within +-12 of them, prox at a different phase per layer"""
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed + 17 * L + 10)
    out = []
    for b, _ in dcases.layers(ref, rows, cols, channels, L, seed):
        near = np.clip(b.astype(np.int64) + rng.integers(-12, 13, size=b.shape), 0, 255).astype(np.uint8)
        out.append((b, near, prox_plane(rows, cols, 5 * len(out) + seed + 1, rng)))
    return out


# ---------------------------------------------------------------------------------------------------
# the aliased shift scene
# ---------------------------------------------------------------------------------------------------
SHIFT_ROWS, SHIFT_COLS, SHIFT_MARGIN = 24, 40, 8
# fine pixels by which frame n's view of the texture is displaced: all four phases modulo 2, five of the nine modulo 3
SHIFT_DISPLACEMENTS = [(1, 0), (0, 1), (0, 0), (1, 1), (2, 3)]


def _gauss_filter(a, sigma=1.0, radius=4):
    k = np.exp(-0.5 * (np.arange(-radius, radius + 1) / sigma) ** 2)
    k /= k.sum()
    p = np.pad(a, radius, mode="wrap")
    rows = sum(k[i] * p[i:i + a.shape[0]] for i in range(2 * radius + 1))
    return sum(k[i] * rows[:, i:i + a.shape[1]] for i in range(2 * radius + 1))


def shift_texture(scale, channels, seed):
    """T: Gaussian-filtered seeded noise, sigma = 1 fine pixel, scaled into 32 .. 223, on scale * 24 x scale * 40 plus a margin"""
    rng = np.random.default_rng(8000 + seed)
    shape = (scale * SHIFT_ROWS + 2 * SHIFT_MARGIN, scale * SHIFT_COLS + 2 * SHIFT_MARGIN)
    planes = []
    for _ in range(channels):
        g = _gauss_filter(rng.standard_normal(shape))
        planes.append(32.0 + 191.0 * (g - g.min()) / (g.max() - g.min()))
    return planes[0] if channels == 1 else np.stack(planes, axis=-1)


def shift_clip(scale, channels=3, seed=0, noise=6, q=2, radius=2, strength=spec.STRENGTH_DEFAULT, name=None):
    """the aliased shift scene: frame n = rint of the scale x scale box mean of T displaced by SHIFT_DISPLACEMENTS[n] fine pixels, plus seeded
    integer noise in [-noise, noise]; constant depth 4, identity rotations, K = (32, 32, 20, 12), camera centres that displace frame n by exactly
    (dx_n, dy_n) / scale source pixels (denoise_cases.shift_clean's construction with fractional steps); the path is the chain itself.
    case["truth"]: T on frame q's fine grid"""
    T = shift_texture(scale, channels, seed)
    rng = np.random.default_rng(8500 + seed)
    rows, cols, mg = SHIFT_ROWS, SHIFT_COLS, SHIFT_MARGIN
    frames = []
    for dx, dy in SHIFT_DISPLACEMENTS:
        part = T[mg + dy:mg + dy + scale * rows, mg + dx:mg + dx + scale * cols]
        box = part.reshape((rows, scale, cols, scale) + part.shape[2:]).mean(axis=(1, 3))
        frames.append((np.rint(box).astype(np.int64) + rng.integers(-noise, noise + 1, size=box.shape)).astype(np.uint8))
    n = len(frames)
    depth = np.full((rows, cols), 4.0)
    R, t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
    A = np.stack([np.eye(3)] * n)
    c = np.array([[dx / scale * 4.0 / 32.0, dy / scale * 4.0 / 32.0, 0.0] for dx, dy in SHIFT_DISPLACEMENTS])
    case = _with_scale(dcases._clip(name or "shift-%s-x%d-%d" % ("bgr" if channels == 3 else "gray", scale, seed), frames, [depth] * n, [R] * n, [t] * n,
                                    (32.0, 32.0, 20.0, 12.0), A, c, A, c, np.ones(n), q, radius, strength), scale)
    dx, dy = SHIFT_DISPLACEMENTS[q]
    case["truth"] = T[mg + dy:mg + dy + scale * rows, mg + dx:mg + dx + scale * cols]
    return case


# ---------------------------------------------------------------------------------------------------
# clips for the frame and the clip call
# ---------------------------------------------------------------------------------------------------
def _with_scale(case, scale, name=None):
    case = dict(case, scale=int(scale), occlusion=0, search=0, tol_q16=0)
    if name:
        case["name"] = name
    return case


def all_cases(pose_table):
    """-> list of frame cases, names unique: the aliased shift scene, gray and BGR, at scale 2 and 3; a fold clip (parallax: some patch weights
    are 0) plain and through a zoomed window; the gained neighbours with the gain on and off; a smooth clip of five sources at radius 2 from its
    middle and, one-sided, from its first frame, at scale 1; one source alone at scale 4; the 2 x 2 dense case"""
    h = 24 - 5
    five = scases.smooth_clip(17, 33, 1, 21, t=1.0, shutter=0.0, samples=1, nsources=5)
    fs = dcases.from_shutter
    out = [shift_clip(2, 3, 0), shift_clip(2, 1, 1), shift_clip(3, 3, 0), shift_clip(3, 1, 1),
           _with_scale(fs(scases.fold_clip(24, 40, 3), "fold-plain", 0, radius=1), 2),
           _with_scale(fs(scases.fold_clip(24, 40, 1), "fold-zoom", 1, radius=1, window=(2, 3, h, (h * 40) // 24), strength=255), 3),
           _with_scale(fs(scases.smooth_clip(19, 35, 3, 11, t=1.0, shutter=0.0, samples=1, nsources=3), "gained", 1, radius=1, strength=20, min_overlap=64), 2),
           _with_scale(fs(five, "five-middle", 2, radius=2), 2), _with_scale(fs(five, "five-first", 0, radius=2, strength=1), 1),
           _with_scale(fs(scases.smooth_clip(9, 21, 3, 22, t=0.0, shutter=0.0, samples=1, nsources=1), "one-source", 0), 4),
           _with_scale(fs(scases.dense_clip(pose_table, "2x2", 2, 2, 3, holes=0.0), "2x2", 1, radius=1), 2)]
    g = out[6]
    fr = g["frames"]
    g["frames"] = [np.clip(fr[0].astype(np.int64) * 5 // 4, 0, 255).astype(np.uint8), fr[1], np.clip(fr[2].astype(np.int64) * 4 // 5, 0, 255).astype(np.uint8)]
    out.insert(7, dict(g, name="gain-off", gain_mode=1))
    assert len({c["name"] for c in out}) == len(out)
    return out


sources_and_poses = dcases.sources_and_poses


def run_spec(case, q=None):
    """the definition on frame q of a case.  -> superres_frame's dict plus sources"""
    src, M, m = sources_and_poses(case, q)
    pick = lambda k: [case[k][n] for n in src]
    r = spec.superres_frame(pick("frames"), pick("depths"), pick("Rs"), pick("ts"), case["K"], M, m, case["scale"], case["window"], case["strength"], case["min_overlap"],
                            case["gain_mode"], case["mode"], case["q5_mode"], case["iterations"])
    return dict(r, sources=src)


def seen_by_all(r):
    """the fine pixels every source of a frame result sees"""
    ok = np.ones(r["planes"][0]["prox"].shape, dtype=bool)
    for p in r["planes"]:
        ok &= p["prox"] != 0
    return ok


def quality_ratio(case):
    """mean |out - truth| over the fine pixels seen by every source, as a fraction of the one-source call's (the bilinear upscale of the own frame)"""
    r = run_spec(case)
    src, M, m = sources_and_poses(case)
    one = spec.superres_frame([case["frames"][src[0]]], [case["depths"][src[0]]], [case["Rs"][src[0]]], [case["ts"][src[0]]], case["K"], M[:1], m[:1], case["scale"],
                              case["window"], case["strength"], case["min_overlap"], case["gain_mode"], case["mode"], case["q5_mode"], case["iterations"])
    ok = seen_by_all(r)
    assert ok.mean() > 0.5 and np.array_equal(one["image"], r["planes"][0]["bil"])
    err = lambda img: np.abs(img.astype(np.float64) - case["truth"])[ok].mean()
    return err(r["image"]) / err(one["image"]), r
