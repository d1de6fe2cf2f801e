"""Inputs of the clean plate's tests (tests/test_plate_cpu.py, tests/test_gpu_plate.py) and of its golden fixture
(tests/golden/make_golden_plate.py): the layer counts at which the median's kernel takes another instance, the constructed cases with known
answers, the seeded random campaign, the denoise's small solved clips (tests/denoise_cases.py, reused as they are) with the plate's
parameters, and the scene with a mover that shows what the feature is for."""
import numpy as np

import denoise_cases as dcases
import plate_spec_numpy as spec
import retime_cases as rcases

ACC_SHAPES = dcases.ACC_SHAPES
# both ends, even and odd numbers of candidates, and the last count of an instance of the kernel and the first of the next (the instances hold
# 0, 2, 4, 7 and 14 layers)
LAYER_COUNTS = [0, 1, 2, 3, 4, 5, 7, 8, 13, 14]
INSTANCE_SIZES = [0, 2, 4, 7, 14]
RECORD_KEYS = ["plain", "low", "high", "small", "zero"]


def layer_records(channels, L, phase=0):
    """(L, 8) uint64: denoise_cases.records' five cases in turn -- both gain clamps, a plain gain, too small an overlap, a layer sum of 0"""
    rec = dcases.records(channels)
    return np.array([rec[RECORD_KEYS[(j + phase) % 5]] for j in range(L)], dtype=np.uint64).reshape(L, 8)


def median_inputs(shape, channels, L, seed=0):
    """reference and L layers with random bytes under empty mask bytes and mask values other than 0 / 1 (denoise_cases.reference / layers)"""
    ref, rmask = dcases.reference(*shape, channels, seed)
    return ref, rmask, dcases.layers(ref, *shape, channels, L, seed)


def median_parameters(shape, L):
    """(threshold, min_votes) that change with the shape and the layer count"""
    return [24, 1, 255, 12, 60][(shape[0] + L) % 5], 1 + (shape[1] + 2 * L) % min(L + 2, 15)


def random_case(rng):
    """one case of the seeded campaign: a shape up to 40 x 140, channels, a layer count, sparse to dense masks, records or none, parameters"""
    rows, cols = int(rng.integers(2, 41)), int(rng.integers(2, 141))
    ch = int(rng.choice([1, 3]))
    L = int(rng.integers(0, 15))
    shape = (rows, cols) if ch == 1 else (rows, cols, 3)
    ref = rng.integers(0, 256, size=shape, dtype=np.uint8)
    mask = lambda: (rng.integers(0, 256, size=(rows, cols)) * (rng.random((rows, cols)) < rng.random())).astype(np.uint8)
    rmask = mask()
    layers = []
    for _ in range(L):
        near = np.clip(ref.astype(np.int64) + rng.integers(-int(rng.integers(0, 40)) - 1, int(rng.integers(0, 40)) + 2, size=shape), 0, 255).astype(np.uint8)
        layers.append((near if rng.random() < 0.7 else rng.integers(0, 256, size=shape, dtype=np.uint8), mask()))
    records = layer_records(ch, L, int(rng.integers(0, 5))) if L and rng.random() < 0.7 else None
    return dict(ref=ref, rmask=rmask, layers=layers, records=records, min_overlap=int(rng.choice([0, 1024, 6000])), gain_mode=int(rng.random() < 0.2),
                threshold=int(rng.integers(1, 256)), min_votes=int(rng.integers(1, 16)))


def spec_of(case):
    return spec.median(case["ref"], case["rmask"], case["layers"], None if case["records"] is None else list(case["records"]), case["min_overlap"] or spec.MIN_OVERLAP_DEFAULT,
                       case["gain_mode"], case["threshold"], case["min_votes"])


# ---------------------------------------------------------------------------------------------------
# constructed cases with known answers: the same list for the definition (CPU) and the kernel (GPU)
# ---------------------------------------------------------------------------------------------------
def _case(name, ref, rmask, layers, want, records=None, min_overlap=0, gain_mode=0, threshold=spec.THRESHOLD_DEFAULT, min_votes=spec.MIN_VOTES_DEFAULT):
    return dict(name=name, ref=ref, rmask=rmask, layers=layers, records=records, min_overlap=min_overlap, gain_mode=gain_mode, threshold=threshold, min_votes=min_votes,
                want=want)


def impulse_flags(rows, cols, y, x, threshold):
    """the flag plane of a frame whose own pixel (y, x) differs from its median by 255 in every channel while every other pixel equals its
    median, every mask set: about p' in the 3 x 3 window of (y, x) D = 255 CH and N = CH k, k the pixels of p's own window inside the frame
    (9, 6 at an edge, 4 in a corner), so p' is moving iff 255 > threshold k; everything else is static"""
    want = np.ones((rows, cols), dtype=np.uint8)
    for py in range(max(y - 1, 0), min(y + 2, rows)):
        for px in range(max(x - 1, 0), min(x + 2, cols)):
            k = (min(py + 2, rows) - max(py - 1, 0)) * (min(px + 2, cols) - max(px - 1, 0))
            want[py, px] = 2 if 255 > threshold * k else 1
    return want


def constructed(channels, impulse_shapes=((17, 65), (33, 129))):
    """-> list of cases, each with `want`: the outputs known by hand (any of image, mask, votes, moving, counts)"""
    rng = np.random.default_rng(77 + channels)
    rows, cols = 19, 70
    npix = rows * cols
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    full, empty = np.full((rows, cols), 7, dtype=np.uint8), np.zeros((rows, cols), dtype=np.uint8)
    base = rng.integers(0, 256, size=shape, dtype=np.uint8)
    ones, votes15 = np.ones((rows, cols), dtype=np.uint8), np.full((rows, cols), 15, dtype=np.uint8)
    out = [_case("all-equal", base, full, [(base, full)] * 14, dict(image=base, mask=ones, votes=votes15, moving=ones, counts=[0, npix, 0, 0]))]
    # one layer 255 away among fourteen equal candidates: the plate is unchanged, whichever layer it is
    v = np.where(rng.random(shape) < 0.5, 0, 255).astype(np.uint8)
    for at in (0, 6, 13):
        ls = [(v, full)] * 14
        ls[at] = ((255 - v).astype(np.uint8), full)
        out.append(_case("one-outlier-at-%d" % at, v, full, ls, dict(image=v, mask=ones, votes=votes15, moving=ones)))
    # the same outlier as the own frame: the plate is the others' value and the own frame is moving everywhere
    out.append(_case("own-outlier", (255 - v).astype(np.uint8), full, [(v, full)] * 14, dict(image=v, moving=np.full((rows, cols), 2, dtype=np.uint8), counts=[0, 0, npix, 0])))
    # two candidates: the lower median is the smaller
    other = rng.integers(0, 256, size=shape, dtype=np.uint8)
    out.append(_case("two-candidates", base, full, [(other, full)], dict(image=np.minimum(base, other), votes=np.full((rows, cols), 2, dtype=np.uint8)), min_votes=2))
    out.append(_case("two-layers-no-own", base, empty, [(other, full), (base, full)], dict(image=np.minimum(base, other), mask=ones, moving=empty, counts=[npix, 0, 0, 0])))
    if channels == 3:  # ties in one channel but not in another: (5, 5, 9, 9) -> 5, (1, 2, 3, 4) -> 2, (7, 7, 7, 7) -> 7
        px = lambda b, g_, r: np.broadcast_to(np.array([b, g_, r], dtype=np.uint8), shape).copy()
        out.append(_case("ties", px(9, 3, 7), full, [(px(5, 1, 7), full), (px(9, 4, 7), full), (px(5, 2, 7), full)], dict(image=px(5, 2, 7), votes=np.full((rows, cols), 4, dtype=np.uint8))))
    # an own mask that is empty while the layers are set: the plate is set, the flags are all 0
    ls = [(rng.integers(0, 256, size=shape, dtype=np.uint8), full) for _ in range(3)]
    med = np.sort(np.stack([i for i, _ in ls]).astype(np.int64), axis=0)[1].astype(np.uint8)
    out.append(_case("own-mask-empty", base, empty, ls, dict(image=med, mask=ones, votes=np.full((rows, cols), 3, dtype=np.uint8), moving=empty, counts=[npix, 0, 0, 0])))
    # min_votes 15 with fewer layers: every own pixel is undecided; min_votes 1 without layers: the plate is the own frame and static
    threes = np.full((rows, cols), 3, dtype=np.uint8)
    out.append(_case("min-votes-15", base, full, ls, dict(moving=threes, counts=[0, 0, 0, npix]), min_votes=15))
    out.append(_case("min-votes-15-reached", base, full, [(base, full)] * 14, dict(moving=ones), min_votes=15))
    out.append(_case("min-votes-1", base, full, [], dict(image=base, mask=ones, votes=ones, moving=ones, counts=[0, npix, 0, 0]), min_votes=1))
    out.append(_case("min-votes-default-no-layers", base, full, [], dict(image=base, moving=threes)))
    # the impulse at every corner and edge midpoint of every tile and of the frame: the halo; thresholds 1, 24, 40 (edges and corners only) and 255
    for ishape in impulse_shapes:
        r_, c_ = ishape
        zero = np.zeros(ishape if channels == 1 else ishape + (3,), dtype=np.uint8)
        set_ = np.ones(ishape, dtype=np.uint8)
        for k, (y, x) in enumerate(dcases.impulse_positions(r_, c_)):
            own = zero.copy()
            own[y, x] = 255
            threshold = [24, 40, 1, 255][k % 4]
            out.append(_case("impulse-%dx%d-%d-%d-t%d" % (r_, c_, y, x, threshold), own, set_, [(zero, set_)] * 4,
                             dict(image=zero, moving=impulse_flags(r_, c_, y, x, threshold)), threshold=threshold))
    return out


# ---------------------------------------------------------------------------------------------------
# the denoise's clips with the plate's parameters
# ---------------------------------------------------------------------------------------------------
def all_cases(pose_table):
    """denoise_cases.all_cases: the noisy shift scene, gray and BGR; the fold pair plain, through the occlusion test and through the search; the
    zoomed window; the gained neighbours with the gain on, off and under too small an overlap; five sources from the middle, one-sided and at
    radius 7; one source; 2 x 2.  The threshold is the case's denoise strength (1 .. 255), min_votes 2 with fewer than three sources"""
    out = []
    for case in dcases.all_cases(pose_table):
        nsrc = len(dcases.sources_and_poses(case)[0])
        out.append(dict(case, threshold=case["strength"], min_votes=3 if nsrc >= 3 else 2))
    return out


def run_spec(case, q=None):
    """the definition on frame q of a case.  -> plate_frame's dict plus sources"""
    src, M, m = dcases.sources_and_poses(case, q)
    pick = lambda k: [case[k][n] for n in src]
    r = spec.plate_frame(pick("frames"), pick("depths"), pick("Rs"), pick("ts"), case["K"], M, m, case["window"], case["threshold"], case["min_votes"], case["min_overlap"],
                         case["gain_mode"], case["occlusion"], case["search"], case["tol_q16"], case["mode"], case["q5_mode"], case["iterations"])
    return dict(r, sources=src)


# ---------------------------------------------------------------------------------------------------
# what the feature is for
# ---------------------------------------------------------------------------------------------------
MOVER_COLS, MOVER_NOISE, MOVER_THRESHOLD = 96, 6, 12
MOVER_ROWS, MOVER_HEIGHT, MOVER_WIDTH = (6, 14), 8, 6   # rows 6 .. 13, six columns
MOVER_TARGET_COLUMNS = [20, 30, 40, 50, 60]             # where source n's block shows in frame q's camera: four columns apart


def mover_scene():
    """the denoise's shift scene, five frames of 96 columns with noise of +-6, and a block of constant 255 pasted into every noisy frame so that
    in frame q = 2's camera (frame n shows SHIFT (n - q) columns on) the five footprints sit at MOVER_TARGET_COLUMNS.
    -> (case, footprints (5, rows, cols) bool in frame q's camera, by source index)"""
    case = dcases.shift_clip(seed=3, channels=3, q=2, radius=2, noise=MOVER_NOISE, name="mover", nframes=5, cols=MOVER_COLS)
    rows = case["depths"][0].shape[0]
    frames, prints = [], np.zeros((5, rows, MOVER_COLS), dtype=bool)
    for n, frame in enumerate(case["frames"]):
        x = MOVER_TARGET_COLUMNS[n] - rcases.SHIFT * (n - case["q"])  # the block's column in frame n itself
        assert 0 <= x and x + MOVER_WIDTH <= MOVER_COLS
        frame = frame.copy()
        frame[MOVER_ROWS[0]:MOVER_ROWS[1], x:x + MOVER_WIDTH] = 255
        frames.append(frame)
        prints[n, MOVER_ROWS[0]:MOVER_ROWS[1], MOVER_TARGET_COLUMNS[n]:MOVER_TARGET_COLUMNS[n] + MOVER_WIDTH] = True
    return dict(case, frames=frames, gain_mode=1, threshold=MOVER_THRESHOLD, min_votes=spec.MIN_VOTES_DEFAULT), prints
