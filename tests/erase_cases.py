"""Inputs of the mover removal's tests (tests/test_erase_cpu.py, tests/test_gpu_erase.py) and of its golden fixture
(tests/golden/make_golden_erase.py): the shapes at which the matte's row segments, its halo, its column reach and the composite's tile can go
wrong, the parameter sets, the flag and composite generators, the constructed flags, the seeded random campaign, the plate's small solved clips
(tests/plate_cases.py, reused as they are) with the matte's parameters, and the scene with a mover that shows what the feature is for."""
import numpy as np

import denoise_cases as dcases
import erase_spec_numpy as spec
import plate_cases as pcases
import retime_cases as rcases

ACC_SHAPES = dcases.ACC_SHAPES
# the row pass owns segments of 1024 pixels with a halo of up to 29: one under, exactly one, one over, two and a rest; and frames lower than the
# column pass's reach of up to 26 rows on either side, at cols % 4 != 0 and == 0
MATTE_SHAPES = ACC_SHAPES + [(3, 1023), (3, 1024), (3, 1025), (2, 2050), (60, 5), (29, 4)]
MATTE_PARAMETERS = [(0, 0, 1), (2, 2, 4), (3, 8, 16), (1, 0, 7), (0, 8, 3), (3, 0, 1)]  # (open, grow, feather)
FEATHERS = [1, 3, 4, 7, 16]
SEED_DENSITIES = [0.3, 0.7, 0.95]
SEGMENT, TILE_ROWS, TILE_COLS = 1024, 16, 64


# ---------------------------------------------------------------------------------------------------
# the matte
# ---------------------------------------------------------------------------------------------------
def random_flag(shape, seed=0, density=None):
    """flag bytes from 0 .. 255 -- most of them no seed, values above 3 among them --, seeds (2; one in seven 3) sprinkled at the density, solid
    rectangles of 2 and one of 3, a few holes punched back, in six of ten flags a side of the frame without any seed, and one solid block
    of 2 that keeps a core under open = 3"""
    rng = np.random.default_rng(9100 + 131 * seed + shape[0] * 7 + shape[1])
    rows, cols = shape
    density = SEED_DENSITIES[seed % 3] if density is None else density
    F = rng.integers(0, 256, size=shape, dtype=np.uint8)
    sprinkle = rng.random(shape) < density
    F[sprinkle] = np.where(rng.random(shape) < 1.0 / 7.0, 3, 2)[sprinkle]
    for value in (2, 2, 3):
        h, w = int(rng.integers(1, max(rows // 2, 9) + 1)), int(rng.integers(1, max(cols // 2, 9) + 1))
        y, x = int(rng.integers(-2, max(rows - h, 0) + 3)), int(rng.integers(-2, max(cols - w, 0) + 3))
        F[max(y, 0):max(y + h, 0), max(x, 0):max(x + w, 0)] = value
    holes = rng.random(shape) < 0.01
    F[holes] = rng.choice(np.array([0, 1, 4, 130, 255], dtype=np.uint8), size=shape)[holes]
    if rng.random() < 0.6:  # a quiet side without any seed, so that the matte also falls to 0
        quiet = F[:, int(cols * rng.uniform(0.25, 0.6)):]
        quiet[(quiet == 2) | (quiet == 3)] = 1
    # one solid block of 2 of 8 .. 12 pixels a side (cut by the frame, which vetoes nothing) over everything else: a core under every open
    h, w = int(rng.integers(8, 13)), int(rng.integers(8, 13))
    y, x = int(rng.integers(-2, max(rows - h, 0) + 3)), int(rng.integers(-2, max(cols - w, 0) + 3))
    F[max(y, 0):max(y + h, 0), max(x, 0):max(x + w, 0)] = 2
    return F


def single_seed_positions(rows, cols):
    """the frame's corners and both sides of the first tile border in either direction and of every row-segment border, inside the frame, unique"""
    ys = {0, rows - 1} | {y for y in (TILE_ROWS - 1, TILE_ROWS) if y < rows}
    xs = {0, cols - 1} | {x for x in (TILE_COLS - 1, TILE_COLS) if x < cols} | {x for x0 in range(SEGMENT, cols, SEGMENT) for x in (x0 - 1, x0)}
    return sorted((y, x) for y in ys for x in xs)


CONSTRUCTED_SHAPE = (18, 2050)


def constructed_flags():
    """-> list of (name, flag, parameter sets, want or None): `want` the matte known by hand for the FIRST parameter set"""
    rows, cols = CONSTRUCTED_SHAPE
    out = []
    yy, xx = np.mgrid[0:rows, 0:cols]
    for y, x in single_seed_positions(rows, cols):
        F = np.ones(CONSTRUCTED_SHAPE, dtype=np.uint8)
        F[y, x] = 2
        # open 0, grow 2, feather 3: C = 5, a = clamp(5 - chessboard distance, 0, 3)
        want = np.clip(5 - np.maximum(np.abs(yy - y), np.abs(xx - x)), 0, 3).astype(np.uint8)
        out.append(("seed-%d-%d" % (y, x), F, [(0, 2, 3), (0, 8, 16)], want))
    full = lambda T: np.full(CONSTRUCTED_SHAPE, T, dtype=np.uint8)
    out.append(("all-seeds", np.full(CONSTRUCTED_SHAPE, 2, dtype=np.uint8), [(3, 8, 16), (0, 0, 1), (2, 2, 4)], full(16)))
    out.append(("all-undecided", np.full(CONSTRUCTED_SHAPE, 3, dtype=np.uint8), [(3, 8, 16), (2, 2, 4)], full(0)))
    out.append(("no-seeds", np.ones(CONSTRUCTED_SHAPE, dtype=np.uint8), [(0, 8, 16), (3, 8, 16)], full(0)))
    # a block of (o + 1)^2 seeds in every corner survives open = o: nothing outside the frame vetoes
    F = np.zeros(CONSTRUCTED_SHAPE, dtype=np.uint8)
    for ys in (slice(0, 4), slice(rows - 4, rows)):
        for xs in (slice(0, 4), slice(cols - 4, cols)):
            F[ys, xs] = 2
    d = np.maximum(np.minimum(yy, rows - 1 - yy), np.minimum(xx, cols - 1 - xx))  # under open = 3 the core is the four corner pixels
    out.append(("corner-blocks", F, [(3, 1, 2), (2, 2, 4)], np.clip(6 - d, 0, 2).astype(np.uint8)))
    return out


def random_matte_case(rng):
    """one case of the seeded campaign: a shape up to 40 x 1100, every parameter, a seed density"""
    rows = int(rng.integers(2, 41))
    cols = int(rng.integers(2, 141)) if rng.random() < 0.8 else int(rng.integers(1000, 1101))
    o, g, T = int(rng.integers(0, 4)), int(rng.integers(0, 9)), int(rng.integers(1, 17))
    return dict(flag=random_flag((rows, cols), int(rng.integers(0, 1 << 20)), SEED_DENSITIES[int(rng.integers(0, 3))]), open=o, grow=g, feather=T,
                include_undecided=int(rng.random() < 0.5))


def matte_of(case):
    return spec.matte(case["flag"], case["open"], case["grow"], case["feather"], case["include_undecided"])


# ---------------------------------------------------------------------------------------------------
# the composite
# ---------------------------------------------------------------------------------------------------
def composite_inputs(shape, channels, T, seed=0):
    """the own frame and the plate with random bytes under empty mask bytes and mask values other than 0 / 1 (denoise_cases.reference at two
    seeds), and a matte of patches -- 0 (most of the frame), every value 1 .. T, values above T -- of 2 x 6 pixels so that a thread's four
    pixels are all 0, all set and mixed
    -> (ref, rmask, plate, pmask, matte)"""
    rows, cols = shape
    ref, rmask = dcases.reference(rows, cols, channels, seed)
    plate, pmask = dcases.reference(rows, cols, channels, seed + 50)
    rng = np.random.default_rng(4200 + seed + 17 * T + rows + 3 * cols)
    py, px = (rows + 1) // 2, (cols + 5) // 6
    kind = rng.random((py, px))
    values = np.where(kind < 0.45, 0, np.where(kind < 0.6, T, np.where(kind < 0.7, rng.integers(T, 256, size=(py, px)), rng.integers(0, T + 1, size=(py, px)))))
    matte = np.repeat(np.repeat(values, 2, axis=0), 6, axis=1)[:rows, :cols].astype(np.uint8)
    return ref, rmask, plate, pmask, np.ascontiguousarray(matte)


def exhaustive_composite(T):
    """a gray frame that holds every (a, R, P), a = 0 .. T, every mask set -> (ref, rmask, plate, pmask, matte), (T + 1) 64 x 1024"""
    a, R, P = np.meshgrid(np.arange(T + 1), np.arange(256), np.arange(256), indexing="ij")
    shape = ((T + 1) * 64, 1024)
    u8 = lambda x: np.ascontiguousarray(x.reshape(shape).astype(np.uint8))
    ones = np.ones(shape, dtype=np.uint8)
    return u8(R), ones, u8(P), ones.copy(), u8(a)


def random_composite_case(rng):
    rows, cols = int(rng.integers(2, 41)), int(rng.integers(2, 141))
    ch, T = int(rng.choice([1, 3])), int(rng.integers(1, 17))
    ref, rmask, plate, pmask, matte = composite_inputs((rows, cols), ch, T, int(rng.integers(0, 1000)))
    return dict(ref=ref, rmask=rmask, plate=plate, pmask=pmask, matte=matte, feather=T)


def composite_of(case):
    return spec.composite(case["ref"], case["rmask"], case["plate"], case["pmask"], case["matte"], case["feather"])


# ---------------------------------------------------------------------------------------------------
# the plate's clips with the matte's parameters
# ---------------------------------------------------------------------------------------------------
FRAME_PARAMETERS = [(2, 2, 4, 0), (0, 0, 1, 0), (1, 2, 4, 1), (0, 3, 7, 0), (1, 0, 16, 1), (3, 8, 16, 0), (0, 1, 3, 1)]  # (open, grow, feather, include_undecided)


def all_cases(pose_table):
    """plate_cases.all_cases, every case with one of FRAME_PARAMETERS in turn: the defaults, no cleaning at all, the undecided pixels as seeds"""
    out = []
    for k, case in enumerate(pcases.all_cases(pose_table)):
        o, g, T, und = FRAME_PARAMETERS[k % len(FRAME_PARAMETERS)]
        out.append(dict(case, open=o, grow=g, feather=T, include_undecided=und))
        if case["name"] == "one-source":  # every own pixel undecided: as seeds the matte is full and the plate, which is the own frame, replaces it
            out.append(dict(case, name="one-source-undecided", open=1, grow=2, feather=4, include_undecided=1))
    return out


def run_spec(case, q=None):
    """the definition on frame q of a case.  -> erase_frame's dict plus sources"""
    src, M, m = dcases.sources_and_poses(case, q)
    pick = lambda k: [case[k][n] for n in src]
    r = spec.erase_frame(pick("frames"), pick("depths"), pick("Rs"), pick("ts"), case["K"], M, m, case["window"], case["open"], case["grow"], case["feather"],
                         case["include_undecided"], case["threshold"], case["min_votes"], case["min_overlap"], case["gain_mode"], case["occlusion"], case["search"],
                         case["tol_q16"], case["mode"], case["q5_mode"], case["iterations"])
    return dict(r, sources=src)


# ---------------------------------------------------------------------------------------------------
# what the feature is for
# ---------------------------------------------------------------------------------------------------
MOVER_COLS, MOVER_NOISE, MOVER_THRESHOLD = 96, 6, 12
MOVER_ROWS, MOVER_HEIGHT, MOVER_WIDTH = (7, 17), 10, 8  # rows 7 .. 16, eight columns
MOVER_TARGET_COLUMNS = [20, 30, 40, 50, 60]             # where source n's block shows in frame q's camera: two columns apart
MOVER_PARAMETERS = [(2, 2, 4), (1, 2, 4), (0, 0, 1), (2, 1, 7)]  # the defaults first
HOT_PIXEL = (3, 74)  # seen by four of the five sources, 27 columns from the own footprint


def mover_scene(hot_pixel=False):
    """the plate's mover scene (plate_cases.mover_scene) with a block of 10 rows x 8 columns: the denoise's shift scene, five frames of 96
    columns with noise of +-6, a block of constant 255 pasted into every noisy frame so that in frame q = 2's camera the five footprints sit at
    MOVER_TARGET_COLUMNS.  hot_pixel: one pixel of the own frame at HOT_PIXEL set, per channel, to 255 where the clean byte is below 128 and
    to 0 elsewhere -- at least 128 - 6 from every inlier.
    -> (case, footprints (5, rows, cols) bool in frame q's camera, by source index)"""
    case = dcases.shift_clip(seed=3, channels=3, q=2, radius=2, noise=MOVER_NOISE, name="mover", nframes=5, cols=MOVER_COLS)
    rows = case["depths"][0].shape[0]
    frames, prints = [], np.zeros((5, rows, MOVER_COLS), dtype=bool)
    for n, frame in enumerate(case["frames"]):
        x = MOVER_TARGET_COLUMNS[n] - rcases.SHIFT * (n - case["q"])  # the block's column in frame n itself
        assert 0 <= x and x + MOVER_WIDTH <= MOVER_COLS and MOVER_ROWS[1] <= rows
        frame = frame.copy()
        frame[MOVER_ROWS[0]:MOVER_ROWS[1], x:x + MOVER_WIDTH] = 255
        if hot_pixel and n == case["q"]:
            frame[HOT_PIXEL] = np.where(case["clean"][n][HOT_PIXEL] < 128, 255, 0)
        frames.append(frame)
        prints[n, MOVER_ROWS[0]:MOVER_ROWS[1], MOVER_TARGET_COLUMNS[n]:MOVER_TARGET_COLUMNS[n] + MOVER_WIDTH] = True
    return dict(case, frames=frames, gain_mode=1, threshold=MOVER_THRESHOLD, min_votes=spec.plate.MIN_VOTES_DEFAULT, open=spec.OPEN_DEFAULT, grow=spec.GROW_DEFAULT,
                feather=spec.FEATHER_DEFAULT, include_undecided=0), prints
