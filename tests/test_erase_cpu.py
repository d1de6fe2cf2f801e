"""GPU-free tests of the mover removal (include/rsdsfm_erase.h): the definition (tests/erase_spec_numpy.py) against its golden fixture, the matte
against a plain per-pixel loop and against the blend's seam distance, its identities, the composite exhaustively against exact integer
division, the counters, what the feature is for on a scene with a mover (bounds derived, not measured), the generators' promise, the exported
symbols, the launch counts and the parameter struct.  (The calls' refusals need a context: tests/test_gpu_erase.py.)"""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import erase_cases as cases  # noqa: E402
import erase_spec_numpy as spec  # noqa: E402
import stabilize_blend_spec_numpy as blend  # noqa: E402
from make_golden_erase import PLANES, digest  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_erase_v1.npz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_erase.h")).read()  # what this file tests is declared there: without the header, nothing here runs
NEW_SYMBOLS = {"rsdsfm_erase_params_init", "rsdsfm_mover_matte_dev", "rsdsfm_mover_matte_launches", "rsdsfm_erase_composite_dev", "rsdsfm_erase_composite_launches",
               "rsdsfm_erase_frame_dev", "rsdsfm_erase_launches", "rsdsfm_erase_video_dev"}
ERR_INVALID = -1


def chessboard(a, b):
    """(rows, cols) the chessboard distance from every pixel to the nearest True pixel of b, only where a selects; a large number without any"""
    ys, xs = np.where(b)
    yy, xx = np.mgrid[0:b.shape[0], 0:b.shape[1]]
    d = np.full(b.shape, 1 << 20, dtype=np.int64)
    for y, x in zip(ys, xs):
        d = np.minimum(d, np.maximum(np.abs(yy - y), np.abs(xx - x)))
    return np.where(a, d, 1 << 20)


# ---------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------
def test_spec_equals_the_golden_fixture(oracle):
    g = np.load(GOLDEN)
    all_cases = cases.all_cases(oracle.pose_table)
    assert {k.split("/")[0] for k in g.files} == {c["name"] for c in all_cases}
    seen = np.zeros(5, dtype=np.int64)
    for case in all_cases:
        n = case["name"] + "/"
        assert digest(case) == int(g[n + "digest"]), n
        r = cases.run_spec(case)
        for k in PLANES:
            assert np.array_equal(r[k], g[n + k]), (n, k)
        assert list(r["counts"]) == g[n + "counts"].tolist() and sum(r["counts"]) == r["mask"].size, n
        assert np.array_equal(r["moving"], r["plate"]["moving"]) and np.array_equal(r["mask"], (r["plate"]["ref"][1] != 0).astype(np.uint8)), n
        seen += np.array(r["counts"])
    assert (seen[:4] > 0).all() and seen[4] == 0  # the plate holds the own frame as a candidate: a frame call leaves nothing unresolved
    assert os.path.getsize(GOLDEN) <= 256 * 1024
    assert {(c["open"], c["grow"], c["feather"], c["include_undecided"]) for c in all_cases} >= set(cases.FRAME_PARAMETERS)
    one = cases.run_spec([c for c in all_cases if c["name"] == "one-source-undecided"][0])
    assert np.array_equal(one["image"], one["plate"]["ref"][0]) and one["counts"][2] == int((one["mask"] != 0).sum()) > 0


@pytest.mark.parametrize("include_undecided", [0, 1])
def test_the_matte_against_a_plain_loop(include_undecided):
    """per pixel: the seeds, the window inside the frame, the nearest core pixel by searching every pixel"""
    for k, (o, g, T) in enumerate(cases.MATTE_PARAMETERS):
        F = cases.random_flag((11, 14), seed=k)
        rows, cols = F.shape
        seed = [[F[y, x] == 2 or (include_undecided and F[y, x] == 3) for x in range(cols)] for y in range(rows)]
        core = [[all(seed[v][u] for v in range(max(y - o, 0), min(y + o, rows - 1) + 1) for u in range(max(x - o, 0), min(x + o, cols - 1) + 1)) for x in range(cols)]
                for y in range(rows)]
        C = o + g + T
        want = np.zeros((rows, cols), dtype=np.uint8)
        for y in range(rows):
            for x in range(cols):
                d = min([max(abs(y - v), abs(x - u)) for v in range(rows) for u in range(cols) if core[v][u]] + [C])
                want[y, x] = min(max(C - d, 0), T)
        assert np.array_equal(spec.matte(F, o, g, T, include_undecided), want), (o, g, T)


def test_the_matte_is_two_seam_distances():
    """core = blend.seam_distance(s, o + 1) == o + 1 and d = blend.seam_distance(~core, C), bit for bit: 288 random cases over six shapes"""
    rng = np.random.default_rng(288)
    n = 0
    for shape in ((2, 2), (3, 7), (17, 65), (29, 4), (33, 129), (5, 300)):
        for _ in range(48):
            F = cases.random_flag(shape, int(rng.integers(0, 1 << 20)), float(rng.choice(cases.SEED_DENSITIES)))
            o, g, T, und = int(rng.integers(0, 4)), int(rng.integers(0, 9)), int(rng.integers(1, 17)), int(rng.integers(0, 2))
            s, C = spec.seeds(F, und), o + g + T
            core = blend.seam_distance(s, o + 1) == o + 1
            assert np.array_equal(core, spec.core_of(s, o))
            d = blend.seam_distance(~core, C)
            assert np.array_equal(d, spec.core_distance(core, C)) and np.array_equal(spec.matte(F, o, g, T, und), np.clip(C - d.astype(np.int64), 0, T))
            n += 1
    assert n == 288


def test_the_mattes_identities():
    rng = np.random.default_rng(5)
    for shape in ((2, 2), (17, 65), (29, 4)):
        F = rng.integers(0, 5, size=shape, dtype=np.uint8)
        for und in (0, 1):  # o = g = 0, T = 1: the matte is the seeds
            assert np.array_equal(spec.matte(F, 0, 0, 1, und), spec.seeds(F, und).astype(np.uint8))
        for o, g, T in cases.MATTE_PARAMETERS:  # all seeds: T everywhere
            assert (spec.matte(np.full(shape, 2, dtype=np.uint8), o, g, T) == T).all()
            assert (spec.matte(np.full(shape, 3, dtype=np.uint8), o, g, T) == 0).all() and (spec.matte(np.full(shape, 3, dtype=np.uint8), o, g, T, 1) == T).all()
            assert (spec.matte(np.where(F == 2, 6, F), o, g, T, 1) == spec.matte(np.where(F == 2, 0, F), o, g, T, 1)).all()  # a byte above 3 is no seed
    # one hot pixel's flag, a 3 x 3 block, survives o = 0 and o = 1 (its centre) and vanishes at o = 2; 12 x 12 keeps 8 x 8 at o = 2
    F = np.ones((30, 40), dtype=np.uint8)
    F[10:13, 20:23] = 2
    s = spec.seeds(F)
    assert spec.core_of(s, 0).sum() == 9 and spec.core_of(s, 1).sum() == 1 and spec.core_of(s, 1)[11, 21] and spec.core_of(s, 2).sum() == 0
    assert (spec.matte(F, 2, 8, 16) == 0).all() and spec.matte(F, 1, 0, 1).sum() == 9  # the lone core pixel grown back by o
    F = np.ones((30, 40), dtype=np.uint8)
    F[5:17, 9:21] = 2
    core = spec.core_of(spec.seeds(F), 2)
    assert core.sum() == 64 and core[7:15, 11:19].all()
    a = spec.matte(F, 2, 2, 4)  # T within o + g = 4 of the core, then 3, 2, 1, and 0 from distance 8 on
    d = chessboard(np.ones_like(core), core)
    assert np.array_equal(a, np.clip(8 - d, 0, 4)) and (a[3:19, 7:23] == 4).all() and a[2, 7] == 3 and a[0, 15] == 1 and (a[:, 26:] == 0).all()
    # a mover at the border survives: the window is cut by the frame
    F = np.ones((9, 9), dtype=np.uint8)
    F[0:3, 0:3] = 2
    assert spec.core_of(spec.seeds(F), 2)[0, 0] and spec.core_of(spec.seeds(F), 2).sum() == 1


def test_the_composite_exhaustively_against_exact_division():
    """every (T, a, R, P): Python's integers; a == T gives P and a == 0 gives R exactly; the result lies between R and P; and the kernel's
    reciprocal, (x * ceil(65536 / T)) >> 16, is x // T for every x the formula can produce, within 32 bits"""
    for T in range(1, spec.FEATHER_MAX + 1):
        ref, rmask, plate, pmask, matte = cases.exhaustive_composite(T)
        assert {(int(a), int(r), int(p)) for a, r, p in zip(matte[::64, 0], ref[::64, 0], plate[::64, 0])} == {(a, 0, 0) for a in range(T + 1)}
        assert ref.size == (T + 1) * 65536 and len(np.unique(matte.astype(np.int64) << 16 | ref.astype(np.int64) << 8 | plate)) == ref.size
        got = spec.composite(ref, rmask, plate, pmask, matte, T)
        a, R, P = matte.astype(np.int64), ref.astype(np.int64), plate.astype(np.int64)
        want = np.where(a == 0, R, (2 * (a * P + (T - a) * R) + T - (T & 1)) // (2 * T))  # (x + (T >> 1)) / T in exact integers
        assert np.array_equal(got["image"], want) and (got["mask"] == 1).all()
        assert np.array_equal(got["image"][a == T], plate[a == T]) and np.array_equal(got["image"][a == 0], ref[a == 0])
        assert (got["image"] >= np.minimum(R, P)).all() and (got["image"] <= np.maximum(R, P)).all()  # a rounded convex mix lies between its ends
        assert got["counts"] == [0, 65536, 65536, (T - 1) * 65536, 0]
        x = np.arange(0, 255 * T + (T >> 1) + 1, dtype=np.int64)
        recip = (65536 + T - 1) // T
        assert np.array_equal((x * recip) >> 16, x // T) and int(x[-1]) * recip < 1 << 32, T
    assert spec.composite(np.array([[10, 20]], dtype=np.uint8), [[1, 1]], np.array([[20, 11]], dtype=np.uint8), [[1, 1]], [[1, 1]], 2)["image"].tolist() == [[15, 16]]


@pytest.mark.parametrize("channels", [1, 3])
def test_the_composites_cases_and_counters(channels):
    """per pixel against a plain loop: masks other than 0 / 1, bytes under unset masks, matte bytes above T; the counters sum to rows x cols and
    every one of them occurs"""
    seen = np.zeros(5, dtype=np.int64)
    for T in cases.FEATHERS:
        ref, rmask, plate, pmask, matte = cases.composite_inputs((9, 23), channels, T, seed=T)
        got = spec.composite(ref, rmask, plate, pmask, matte, T)
        R, P, out = spec._planes(ref), spec._planes(plate), spec._planes(got["image"])
        counts = [0] * 5
        for y in range(9):
            for x in range(23):
                a = min(int(matte[y, x]), T)
                kind = 0 if not rmask[y, x] else 1 if a == 0 else 4 if not pmask[y, x] else 2 if a == T else 3
                counts[kind] += 1
                for c in range(channels):
                    r, p = int(R[y, x, c]), int(P[y, x, c])
                    want = 0 if kind == 0 else r if kind in (1, 4) else (a * p + (T - a) * r + T // 2) // T
                    assert out[y, x, c] == want and got["mask"][y, x] == (kind != 0)
        assert got["counts"] == counts and sum(counts) == 9 * 23
        assert (matte > T).any() and (rmask > 1).any() and (pmask > 1).any()
        seen += np.array(counts)
    assert (seen > 0).all()


# ---------------------------------------------------------------------------------------------------
# what the feature is for
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", cases.MOVER_PARAMETERS)
def test_the_mover_is_erased_and_the_rest_keeps_its_bytes(params):
    """The plate's mover scene (five frames, noise +-6, no gain, threshold 12) with a block of 255 of 10 rows x 8 columns whose five footprints
    in frame q's camera are disjoint and two columns apart.  The flag is the own footprint grown by one (the 3 x 3 window), 120 pixels.
    (a) a = T on the own footprint and the output IS the plate there, so |out - clean| <= 6: a median of five with at most two outliers lies
        between inliers (tests/test_plate_cpu.py);
    (b) |out - clean| <= 6 on own + all-five-see: there R (outside every footprint the own frame is within the noise of the clean byte) and P
        are both within 6, and a rounded convex mix of two values lies between them;
    (c) a = 0 and out == R byte for byte at every pixel farther than g + T from the own footprint: the core lies inside the footprint grown by
        1 - o, and a > 0 only within o + g + T - 1 of the core."""
    o, g, T = params
    case, prints = cases.mover_scene()
    case = dict(case, open=o, grow=g, feather=T)
    q, noise = case["q"], cases.MOVER_NOISE
    r = cases.run_spec(case)
    clean = case["clean"][q].astype(np.int64)
    assert r["sources"] == [2, 1, 3, 0, 4] and clean.max() <= 223 and clean.min() >= 32
    own = prints[q]
    assert own.sum() == cases.MOVER_HEIGHT * cases.MOVER_WIDTH == 80 and prints.sum(axis=0).max() == 1
    flagged = r["moving"] == 2
    assert flagged.sum() == 120 and np.array_equal(flagged, chessboard(np.ones_like(own), own) <= 1)
    ref, rmask, _ = r["plate"]["ref"]
    planes = [(ref, rmask)] + r["plate"]["layers"]
    all_five = np.stack([m != 0 for _, m in planes]).all(axis=0)
    assert (all_five & own).sum() == own.sum() and np.array_equal((ref == 255).all(axis=-1) & (rmask != 0), own)
    out = r["image"].astype(np.int64)
    # (a)
    assert (r["matte"][own] == T).all() and np.array_equal(r["image"][own], r["plate"]["image"][own]) and (np.abs(out - clean)[own] <= noise).all()
    assert (np.abs(ref.astype(np.int64) - clean)[own] >= 255 - 223).all()  # the own frame itself still shows the block
    # (b)
    inspect = own | all_five
    assert (np.abs(out - clean)[inspect] <= noise).all() and (r["mask"][inspect] == 1).all()
    # (c)
    far = chessboard(np.ones_like(own), own) > g + T
    assert (r["matte"][far] == 0).all() and np.array_equal(r["image"][far], ref[far]) and np.array_equal(r["mask"], (rmask != 0).astype(np.uint8))
    assert far.sum() > own.size // 4 and inspect.sum() > own.size // 2  # a mask bug cannot empty the test
    assert r["counts"][2] >= own.sum() and r["counts"][4] == 0 and sum(r["counts"]) == own.size


def test_a_hot_pixel_is_kept_at_open_2_and_replaced_at_open_0():
    """one pixel of the own frame at least 122 per channel from every inlier: e >= 366 > 12 * 27, so its whole 3 x 3 window is flagged.  At
    o = 2 the block has no core: the pixel keeps its bytes; at o = 0 it is replaced by the plate, which is within the noise of the clean byte"""
    case, prints = cases.mover_scene(hot_pixel=True)
    y, x = cases.HOT_PIXEL
    clean = case["clean"][case["q"]].astype(np.int64)
    kept = cases.run_spec(dict(case, open=2))
    ref = kept["plate"]["ref"][0]
    block = np.zeros(prints.shape[1:], dtype=bool)
    block[y - 1:y + 2, x - 1:x + 2] = True
    assert np.array_equal(kept["moving"] == 2, block | (chessboard(np.ones_like(block), prints[case["q"]]) <= 1)) and (np.abs(ref[y, x].astype(np.int64) - clean[y, x]) >= 122).all()
    assert (kept["matte"][block] == 0).all() and np.array_equal(kept["image"][y, x], ref[y, x])
    plain = cases.run_spec(cases.mover_scene()[0])
    keep = ~block
    assert np.array_equal(kept["matte"], plain["matte"]) and np.array_equal(kept["image"][keep], plain["image"][keep])  # the speckle changed nothing else
    replaced = cases.run_spec(dict(case, open=0))
    assert (replaced["matte"][block] == case["feather"]).all() and np.array_equal(replaced["image"][y, x], replaced["plate"]["image"][y, x])
    assert (np.abs(replaced["image"][y, x].astype(np.int64) - clean[y, x]) <= cases.MOVER_NOISE).all()


# ---------------------------------------------------------------------------------------------------
# the generators' promise
# ---------------------------------------------------------------------------------------------------
def test_the_generators_give_the_kernels_something_to_do():
    """the campaigns tests/test_gpu_erase.py runs, on the definition alone: at least two thirds of the random matte cases with o > 0 keep a core,
    every matte value 0 .. T occurs for every T reached, and all five counters of the composite are non-zero"""
    rng = np.random.default_rng(20261)
    with_open = with_core = 0
    values = {}
    for _ in range(60):
        case = cases.random_matte_case(rng)
        a = cases.matte_of(case)
        values.setdefault(case["feather"], set()).update(np.unique(a).tolist())
        if case["open"] > 0:
            with_open += 1
            with_core += bool(spec.core_of(spec.seeds(case["flag"], case["include_undecided"]), case["open"]).any())
    assert with_open >= 30 and 3 * with_core >= 2 * with_open, (with_core, with_open)
    assert all(v == set(range(T + 1)) for T, v in values.items()) and len(values) >= 12, values
    seen = np.zeros(5, dtype=np.int64)
    for _ in range(20):
        seen += np.array(cases.composite_of(cases.random_composite_case(rng))["counts"])
    assert (seen > 0).all()
    for shape in cases.MATTE_SHAPES:  # the shapes of the GPU test: on every frame of 8 x 8 or more every parameter set keeps a core somewhere
        for k, (o, g, T) in enumerate(cases.MATTE_PARAMETERS):
            for und in (0, 1):
                a = spec.matte(cases.random_flag(shape, k), o, g, T, und)
                assert min(shape) < 2 * spec.OPEN_MAX + 2 or a.max() == T, (shape, o, g, T, und)
    names = [n for n, _, _, _ in cases.constructed_flags()]
    assert len(names) == len(set(names)) and (0, 0) in cases.single_seed_positions(*cases.CONSTRUCTED_SHAPE)
    assert {(15, 1023), (16, 1024), (17, 2049), (0, 63), (0, 64), (17, 2047), (0, 2048)} <= set(cases.single_seed_positions(*cases.CONSTRUCTED_SHAPE))
    for name, F, params, want in cases.constructed_flags():
        assert want is None or np.array_equal(spec.matte(F, *params[0]), want), name


# ---------------------------------------------------------------------------------------------------
# the host functions
# ---------------------------------------------------------------------------------------------------
def test_symbols_launch_counts_and_params(rsdsfm):
    assert NEW_SYMBOLS == set(rsdsfm.erase_declared_symbols()) and NEW_SYMBOLS <= set(rsdsfm.declared_symbols())
    for arith in ("reference", "fused"):
        lib = rsdsfm.load_library(arith=arith)
        assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
        assert lib.rsdsfm_erase_composite_launches() == 1 and lib.rsdsfm_mover_matte_launches(720, 1280) == 3
    assert rsdsfm.erase_composite_launches() == 1
    for rows, cols in ((2, 2), (37, 67), (720, 1280)):
        assert rsdsfm.mover_matte_launches(rows, cols) == 3
        for nsrc in (1, 2, 5, 15):
            assert rsdsfm.erase_launches(rows, cols, nsrc) == rsdsfm.plate_launches(rows, cols, nsrc) + 3 + 1
    for bad in ((1, 8, 3), (8, 16385, 3), (8, 8, 0), (8, 8, 16)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.erase_launches(*bad)
    for bad in ((1, 8), (8, 16385)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.mover_matte_launches(*bad)
    assert rsdsfm.erase_default_params() == dict(rsdsfm.plate_default_params(), open=2, grow=2, feather=4, include_undecided=0)
    assert "NOT here" in HEADER_TEXT and "choices, not measurements" in HEADER_TEXT and '#include "rsdsfm_plate.h"' in HEADER_TEXT
    assert ctypes.sizeof(rsdsfm.EraseParams) == 72 and rsdsfm._erase_params().struct_bytes == 72
    assert rsdsfm.load_library().rsdsfm_erase_params_init(None) == ERR_INVALID
    p = rsdsfm._erase_params(open=0, grow=0, feather=16)
    assert (p.open, p.grow, p.feather) == (-1, -1, 16) and list(p.reserved) == [0] * 5
    assert (spec.OPEN_DEFAULT, spec.GROW_DEFAULT, spec.FEATHER_DEFAULT) == (2, 2, 4)
    assert (spec.OPEN_MAX, spec.GROW_MAX, spec.FEATHER_MAX) == (rsdsfm.ERASE_OPEN_MAX, rsdsfm.ERASE_GROW_MAX, rsdsfm.ERASE_FEATHER_MAX) == (3, 8, 16)
    assert os.path.exists(rsdsfm.ERASE_HEADER_PATH)
