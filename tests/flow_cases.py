"""Seeded inputs for the DeepFlow front end's edge tests (numpy only): the frame generators, the case tables that
tests/test_gpu_flow_edges.py runs on the GPU and tests/test_flow_cpu.py checks in the spec alone (finite; float32 against float64),
and the random case generator of tests/fuzz_flow.py.

A "kind" is a rule that gives frame i of a clip; a pair is frames 0 and 1.  Every frame is a function of (kind, i, rows, cols, seed)
only, so the CPU tests, the GPU tests and the fuzzer see the same bytes.
"""
import collections
import math

import numpy as np

import flow_spec_numpy as S


def texture(rows, cols, dx=0.0, dy=0.0, seed=0):
    """a smooth four-octave pattern (wavelengths 26 .. 210 px) sampled at (x - dx, y - dy): any sub-pixel translation, any size"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    x, y = x - dx, y - dy
    f = np.full_like(x, 128.0)
    for o in range(4):
        for _ in range(3):
            th, ph = rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
            f += 30.0 / (o + 1) * np.sin(0.03 * 2 ** o * (np.cos(th) * x + np.sin(th) * y) + ph)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def noise(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(rows, cols), dtype=np.uint8)


def checker(rows, cols, shift, cell=4):
    y, x = np.mgrid[0:rows, 0:cols]
    return ((((x - shift) // cell + y // cell) % 2) * 255).astype(np.uint8)


def step(rows, cols, shift):
    x = np.arange(cols)[None, :] + np.zeros((rows, 1), np.int64)
    return np.where(x >= cols // 2 + shift, 255, 0).astype(np.uint8)


# kind -> frame i (gray)
KINDS = {
    "moving": lambda i, r, c, s: texture(r, c, 1.3 * i, -0.8 * i, s),  # 1.5 px per frame
    "far": lambda i, r, c, s: texture(r, c, 12.0 * i, -9.0 * i, s),  # the coarse levels warp well outside the frame
    "still": lambda i, r, c, s: texture(r, c, 0.0, 0.0, s),
    "noise": lambda i, r, c, s: noise(r, c, 1000003 * s + i),  # independent frames
    "texture_noise": lambda i, r, c, s: noise(r, c, 1000003 * s + i) if i % 2 else texture(r, c, 0.0, 0.0, s),
    "constant": lambda i, r, c, s: np.full((r, c), 97, np.uint8),
    "black_white": lambda i, r, c, s: np.full((r, c), 255 if i % 2 else 0, np.uint8),
    "checker": lambda i, r, c, s: checker(r, c, 2 * i),
    "step": lambda i, r, c, s: step(r, c, 3 * i),
}


def to_bgr(g):
    """three channels that differ (B = 255 - g, G = g, R = g // 3): the integer gray of the result is about 0.57 g"""
    return np.stack([255 - g, g, g // 3], axis=-1).astype(np.uint8)


def frame(kind, i, rows, cols, seed=0, channels=1):
    g = KINDS[kind](i, rows, cols, seed)
    return to_bgr(g) if channels == 3 else g


def clip(kind, nframes, rows, cols, seed=0, channels=1):
    return np.stack([frame(kind, i, rows, cols, seed, channels) for i in range(nframes)])


# cls: the class of input whose float32-against-float64 figure DESIGN section 12 records (None: too expensive for the float64 run)
Case = collections.namedtuple("Case", "id kind rows cols channels params cls seed")


def _case(id, kind, rows=70, cols=100, channels=1, params=None, cls="smooth", seed=11):
    return Case(id, kind, rows, cols, channels, dict(params or {}), cls, seed)


def pair(case):
    return tuple(frame(case.kind, i, case.rows, case.cols, case.seed, case.channels) for i in (0, 1))


def frames(case, nframes):
    return clip(case.kind, nframes, case.rows, case.cols, case.seed, case.channels)


_spec_cache = {}


def spec(case, i=0, dtype=np.float32):
    """the spec's field of frames (i, i + 1) of the case's clip, computed once per process"""
    key = (case.id, i, np.dtype(dtype).name)
    if key not in _spec_cache:
        a, b = (frame(case.kind, j, case.rows, case.cols, case.seed, case.channels) for j in (i, i + 1))
        _spec_cache[key] = S.deep_flow(a, b, dtype=dtype, **case.params)
    return _spec_cache[key]


# content: one mid size with 2 x 3 SOR regions on its finest level, default parameters
CONTENT = [
    _case("noise_vs_noise", "noise", cls="noise"),
    _case("texture_vs_noise", "texture_noise", cls="noise"),
    _case("constant", "constant", cls="zero"),
    _case("black_vs_white", "black_white", cls="edges"),
    _case("checker_shift2", "checker", cls="edges"),
    _case("step_shift3", "step", cls="edges"),
    _case("translate_12_9", "far", cls="far"),
    _case("bgr_channels_differ", "moving", channels=3),
]

# parameters over the documented ranges, one at a time, on the moving texture
MIN0 = [_case("min0_down%g" % d, "moving", params=dict(min_size=0, downscale=d)) for d in (0.3, 0.5, 0.74)]  # ran to a 1x1 level before the fix
PARAMS = (
    [_case("sigma0", "moving", params=dict(sigma=0.0)), _case("sigma2", "moving", params=dict(sigma=2.0)),
     _case("sigma16", "moving", params=dict(sigma=16.0), cls="sigma16"),
     _case("min0_down0.8", "moving", params=dict(min_size=0, downscale=0.8))]
    + MIN0
    + [_case("zero_data_term", "moving", params=dict(alpha=20.0, delta=0.0, gamma=0.0), cls="zero"),
       _case("omega0.5", "moving", params=dict(omega=0.5)), _case("omega1.95", "moving", params=dict(omega=1.95))]
    + [_case("sor%d" % n, "moving", params=dict(sor_iterations=n)) for n in (1, 3, 4, 5, 8, 9)]
    + [_case("fixed_point1", "moving", params=dict(fixed_point_iterations=1))]
)

# geometry: the smallest frame, strips, either side of the one-region rule (both sides <= 64), a multiple of the 48-pixel interior
# and one past it; 2 x 5 iterations keep the spec cheap
GEOMETRY = [_case("%dx%d" % (r, c), "moving", r, c, params=dict(fixed_point_iterations=2, sor_iterations=5))
            for r, c in ((2, 2), (2, 40), (3, 200), (300, 3), (64, 64), (64, 65), (65, 64), (96, 96), (97, 49), (112, 113))]

# full sizes: 140 / 405 / 920 SOR regions per launch; downscale 0.5 keeps the pyramid at 1.33 frames of pixels
FULL = [
    _case("480p", "moving", 480, 640, params=dict(downscale=0.5, fixed_point_iterations=2, sor_iterations=6), cls="full"),
    _case("720p", "moving", 720, 1280, params=dict(downscale=0.5, fixed_point_iterations=2, sor_iterations=6), cls="full"),
    _case("1080p", "moving", 1080, 1920, params=dict(downscale=0.5, fixed_point_iterations=1, sor_iterations=5), cls=None),
]

ALL = CONTENT + PARAMS + GEOMETRY + FULL
BY_ID = {c.id: c for c in ALL}
assert len(BY_ID) == len(ALL)

# clips: 4 frames of these through the batched path, plus one whose frames are all identical
CLIPS = [BY_ID[i] for i in ("noise_vs_noise", "translate_12_9", "64x65", "sigma16", "min0_down0.5", "720p")]
STILL = _case("still", "still", cls="zero")


# ---------------------------------------------------------------------------------------------------
# the random campaign (tests/fuzz_flow.py)
# ---------------------------------------------------------------------------------------------------
EDGE_SIDES = (2, 3, 63, 64, 65, 66, 95, 96, 97, 98)


def _side(rng, max_side):
    if rng.random() < 0.35:
        return int(min(rng.choice(EDGE_SIDES), max_side))
    return int(rng.integers(2, max_side + 1))


def _log_uniform(rng, lo, hi):
    return float(math.exp(rng.uniform(math.log(lo), math.log(hi))))


def random_case(n, seed, max_side=200):
    """case n of campaign `seed`: sides in [2, max_side] biased to the edges of the SOR tiling, 1 or 3 channels, a kind of the tables
    above, parameters over the ranges include/rsdsfm_flow.h documents"""
    rng = np.random.default_rng([seed, n])
    rows, cols = _side(rng, max_side), _side(rng, max_side)
    kind = str(rng.choice(sorted(KINDS)))
    p = dict(
        downscale=float(rng.uniform(0.3, 0.97)),
        min_size=int(rng.choice([0, 1, 5, 25])),
        sigma=16.0 if rng.random() < 0.1 else float(rng.uniform(0.0, 4.0)),
        fixed_point_iterations=int(rng.integers(1, 4)),
        sor_iterations=int(rng.integers(1, 10)),
        omega=float(rng.uniform(0.3, 1.95)),
        alpha=_log_uniform(rng, 0.05, 20.0),
        delta=0.0 if rng.random() < 0.2 else _log_uniform(rng, 0.01, 10.0),
        gamma=0.0 if rng.random() < 0.2 else _log_uniform(rng, 0.1, 50.0),
    )
    return Case("fuzz_%d_%d" % (seed, n), kind, rows, cols, int(rng.choice([1, 3])), p, None, int(rng.integers(1 << 20)))
