"""GPU-free tests of the clean plate (include/rsdsfm_plate.h): the definition (tests/plate_spec_numpy.py) against its golden fixture, the
constructed cases with known answers, the order of the layers, the gain, what the feature is for on a scene with a mover (bounds derived, not
measured), the exported symbols, the launch counts and the parameter struct, and synth.render_sequence's mover.  (The calls' refusals need a
context: tests/test_gpu_plate.py.)"""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import denoise_cases as dcases  # noqa: E402
import denoise_spec_numpy as denoise  # noqa: E402
import plate_cases as cases  # noqa: E402
import plate_spec_numpy as spec  # noqa: E402
import shutter_cases as scases  # noqa: E402
from make_golden_plate import digest, median_cases  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_plate_v1.npz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_plate.h")).read()  # what this file tests is declared there: without the header, nothing here runs
NEW_SYMBOLS = {"rsdsfm_plate_params_init", "rsdsfm_plate_median_dev", "rsdsfm_plate_median_launches", "rsdsfm_plate_frame_dev", "rsdsfm_plate_launches",
               "rsdsfm_plate_video_dev"}
ERR_INVALID = -1
PLANES = ("image", "mask", "votes", "moving")


# ---------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------
def test_spec_equals_the_golden_fixture(oracle):
    g = np.load(GOLDEN)
    all_cases = cases.all_cases(oracle.pose_table)
    medians = median_cases()
    assert {k.split("/")[0] for k in g.files} == {c["name"] for c in all_cases} | set(medians)
    seen = np.zeros(4, dtype=np.int64)
    for case in all_cases:
        n = case["name"] + "/"
        assert digest(case) == int(g[n + "digest"]), n
        r = cases.run_spec(case)
        for k in PLANES + ("records",):
            assert np.array_equal(r[k], g[n + k]), (n, k)
        assert list(r["counts"]) == g[n + "counts"].tolist() and sum(r["counts"]) == r["mask"].size, n
        seen += np.array(r["counts"])
    for name, case in medians.items():
        r = cases.spec_of(case)
        for k in PLANES:
            assert np.array_equal(r[k], g[name + "/" + k]), (name, k)
        assert list(r["counts"]) == g[name + "/counts"].tolist(), name
        seen += np.array(r["counts"])
    assert (seen > 0).all()
    assert os.path.getsize(GOLDEN) <= 256 * 1024
    assert {c["frames"][0].ndim for c in all_cases} == {2, 3} and {(c["occlusion"], c["search"]) for c in all_cases} == {(0, 0), (1, 0), (1, 1)}
    assert {len(dcases.sources_and_poses(c)[0]) for c in all_cases} >= {1, 2, 3, 5}
    assert not np.array_equal(g["gained/image"], g["gain-off/image"]) and np.array_equal(g["gain-off/image"], g["gain-small-overlap/image"])


def test_one_source_is_the_window_render(oracle):
    case = [c for c in cases.all_cases(oracle.pose_table) if c["name"] == "one-source"][0]
    r = cases.run_spec(case)
    ref, rmask, _ = r["ref"]
    assert np.array_equal(r["image"], ref) and np.array_equal(r["mask"], rmask) and np.array_equal(r["votes"], rmask)
    assert np.array_equal(r["moving"], 3 * rmask)  # one candidate is below min_votes: undecided wherever the frame is set


@pytest.mark.parametrize("channels", [1, 3])
def test_constructed_cases_have_their_known_answers(channels):
    names = set()
    for case in cases.constructed(channels):
        got = cases.spec_of(case)
        for k, want in case["want"].items():
            assert np.array_equal(np.asarray(got[k]), np.asarray(want)), (case["name"], k)
        assert sum(got["counts"]) == case["rmask"].size
        names.add(case["name"].split("-")[0])
    assert {"all", "one", "own", "two", "min", "impulse"} <= names and (channels == 1 or "ties" in names)


def test_the_impulse_arithmetic():
    """255 > threshold k: at 24 the whole 3 x 3 window moves (216 < 255), at 40 only where the window is cut by the frame (k = 6: 240, k = 4: 160;
    k = 9: 360), at 255 nothing (k >= 4), at 1 everything"""
    assert (cases.impulse_flags(9, 9, 4, 4, 24)[3:6, 3:6] == 2).all() and (cases.impulse_flags(9, 9, 4, 4, 40) == 1).all()
    f = cases.impulse_flags(9, 9, 0, 0, 40)
    assert f[0, 0] == 2 and f[0, 1] == 2 and f[1, 0] == 2 and f[1, 1] == 1 and (f == 2).sum() == 3
    assert (cases.impulse_flags(9, 9, 0, 0, 255) == 1).all() and (cases.impulse_flags(9, 9, 8, 4, 1) == 2).sum() == 6


@pytest.mark.parametrize("channels", [1, 3])
def test_lower_median_against_a_plain_loop(channels):
    """the definition's vectorised median against sorted() per pixel and channel, with every gain clamp and every mask pattern"""
    ref, rmask, ls = cases.median_inputs((5, 5), channels, 7)
    recs = cases.layer_records(channels, 7)
    got = spec.median(ref, rmask, ls, list(recs), min_votes=1)
    R = denoise._planes(ref)
    ks = [denoise.gained(i, denoise.gains(recs[j], channels)) for j, (i, _) in enumerate(ls)]
    for y in range(5):
        for x in range(5):
            for c in range(channels):
                vals = ([int(R[y, x, c])] if rmask[y, x] else []) + [int(ks[j][y, x, c]) for j in range(7) if ls[j][1][y, x]]
                want = sorted(vals)[(len(vals) - 1) >> 1] if vals else 0
                assert denoise._planes(got["image"])[y, x, c] == want and got["votes"][y, x] == len(vals)


@pytest.mark.parametrize("channels", [1, 3])
def test_the_result_does_not_depend_on_the_order_of_the_layers(channels):
    ref, rmask, ls = cases.median_inputs((37, 67), channels, 4)
    recs = cases.layer_records(channels, 4)
    want = spec.median(ref, rmask, ls, list(recs), threshold=30)
    assert min(want["counts"][:3]) > 0
    for perm in itertools.permutations(range(4)):
        got = spec.median(ref, rmask, [ls[i] for i in perm], [recs[i] for i in perm], threshold=30)
        assert all(np.array_equal(got[k], want[k]) for k in PLANES) and got["counts"] == want["counts"], perm


def test_the_gain_is_the_denoises():
    ref, rmask, ls = cases.median_inputs((16, 64), 3, 1)
    full = np.ones((16, 64), dtype=np.uint8)
    for key, rec in dcases.records(3).items():
        for kw in (dict(), dict(gain_mode=1), dict(min_overlap=6000)):
            got = spec.median(np.zeros_like(ref), np.zeros_like(full), [(ls[0][0], full)], [rec], **kw)  # one candidate: the plate is k itself
            assert np.array_equal(got["image"], denoise.gained(ls[0][0], denoise.gains(rec, 3, kw.get("min_overlap", 1024), kw.get("gain_mode", 0))).astype(np.uint8)), key


# ---------------------------------------------------------------------------------------------------
# what the feature is for
# ---------------------------------------------------------------------------------------------------
def test_the_plate_removes_a_mover_and_the_flag_finds_it():
    """The denoise's shift scene, five frames, noise +-6, no gain, threshold 12, and a block of 255 pasted into every noisy frame so that in frame
    q's camera the five footprints are disjoint and at least two columns apart.
    (a) on the own frame's footprint and wherever all five sources see, |plate - clean| <= 6 per channel: a median of five values with at most two
        outliers lies between inliers, each within the noise amplitude of the clean byte;
    (b) a pixel whose whole 3 x 3 window lies in the own footprint is moving: e >= CH (255 - 223 - 6) = 26 CH > 12 CH per pixel;
    (c) a pixel all five see whose 3 x 3 window touches no footprint is static: two values within 6 of the same clean byte differ by at most 12,
        which is not > 12."""
    case, prints = cases.mover_scene()
    q, noise = case["q"], cases.MOVER_NOISE
    r = cases.run_spec(case)
    clean = case["clean"][q].astype(np.int64)
    rows, cols = prints.shape[1:]
    # the scene meets the conditions: the renders are the frames moved by whole columns, so every candidate is a footprint's 255 or within the noise
    assert r["sources"] == [2, 1, 3, 0, 4] and clean.max() <= 223 and clean.min() >= 32
    planes = [r["ref"][:2]] + r["layers"]
    seen = np.stack([m != 0 for _, m in planes])  # by position in r["sources"]
    ordered = prints[r["sources"]]
    for (image, mask), foot in zip(planes, ordered):
        on = mask != 0
        assert np.array_equal((image == 255).all(axis=-1) & on, foot) and foot.sum() == cases.MOVER_HEIGHT * cases.MOVER_WIDTH
        assert (np.abs(image.astype(np.int64) - clean)[on & ~foot] <= noise).all()
    any_print = prints.any(axis=0)
    assert prints.sum(axis=0).max() == 1  # pairwise disjoint
    xs = sorted(int(np.where(p.any(axis=0))[0].min()) for p in prints)
    assert all(b - (a + cases.MOVER_WIDTH) >= 2 for a, b in zip(xs, xs[1:]))  # at least two columns apart
    own = ordered[0]
    assert ((seen[1:] & ~ordered[1:]).sum(axis=0)[own] >= 3).all()  # the own footprint is seen as background by at least three other sources
    all_five = seen.all(axis=0)
    assert (all_five & own).sum() == own.sum()
    # (a)
    inspect = own | all_five
    assert (np.abs(r["image"].astype(np.int64) - clean)[inspect] <= noise).all() and (r["mask"][inspect] == 1).all()
    # (b)
    interior = denoise.box3(own.astype(np.int64)) == 9
    assert interior.sum() == (cases.MOVER_HEIGHT - 2) * (cases.MOVER_WIDTH - 2) and (r["moving"][interior] == 2).all()
    # (c)
    quiet = all_five & (denoise.box3(any_print.astype(np.int64)) == 0)
    assert (r["moving"][quiet] == 1).all()
    assert inspect.sum() >= interior.sum() and quiet.sum() >= interior.sum() and quiet.sum() > rows * cols // 4  # a mask bug cannot empty the test
    # the own frame itself still shows the block: the plate differs from it there by at least 255 - 229
    assert (np.abs(r["image"].astype(np.int64) - r["ref"][0])[own] >= 26).all()


# ---------------------------------------------------------------------------------------------------
# the host functions
# ---------------------------------------------------------------------------------------------------
def test_symbols_and_launch_counts(rsdsfm):
    assert NEW_SYMBOLS == set(rsdsfm.plate_declared_symbols()) and NEW_SYMBOLS <= set(rsdsfm.declared_symbols())
    for arith in ("reference", "fused"):
        lib = rsdsfm.load_library(arith=arith)
        assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
        assert lib.rsdsfm_plate_median_launches() == 1
    assert rsdsfm.plate_median_launches() == 1
    for rows, cols in ((2, 2), (37, 67), (720, 1280)):
        for nsrc in (1, 2, 5, 15):
            assert rsdsfm.plate_launches(rows, cols, nsrc) == nsrc * rsdsfm.stabilize_window_launches(rows, cols) + (nsrc - 1) + 1
    for bad in ((1, 8, 3), (8, 16385, 3), (8, 8, 0), (8, 8, 16)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.plate_launches(*bad)
    assert rsdsfm.plate_default_params() == dict(radius=2, threshold=24, min_votes=3, min_overlap=1024, gain_mode=0, occlusion=0)
    assert "NOT here" in HEADER_TEXT and "RSDSFM_PLATE_LAYERS_MAX 14" in HEADER_TEXT
    assert ctypes.sizeof(rsdsfm.PlateParams) == 56 and rsdsfm._plate_params().struct_bytes == 56
    assert rsdsfm.load_library().rsdsfm_plate_params_init(None) == ERR_INVALID
    assert spec.THRESHOLD_DEFAULT == 24 and spec.MIN_VOTES_DEFAULT == 3 and spec.LAYERS_MAX == rsdsfm.PLATE_LAYERS_MAX == 14


# ---------------------------------------------------------------------------------------------------
# synth
# ---------------------------------------------------------------------------------------------------
def test_render_sequence_without_a_mover_is_unchanged_and_with_one_shows_the_block(rsdsfm):
    """mover=None: the bytes of the call without the argument, for the argument sets tests/denoise_cases.py and tests/shutter_cases.py reach
    render_sequence with (through shutter_cases.smooth_clip: a plain constant motion) and with gains, speeds and noise; with a mover the
    footprints of mover_planes hold render_occluded_pair's block texture before the noise, and everything else is the plain frame"""
    synth = rsdsfm.synth
    K = (40.0, 40.0, 24.0, 16.0)
    v, w = np.array([0.02, 0.0, 0.0]), np.array([0.0, 0.002, 0.0])
    sets = [dict(), dict(gains=[1.0, 1.2, 0.8, 1.0]), dict(noise=6), dict(speeds=[1.0, 1.5, 0.5]), dict(gains=[1.0, 1.1, 0.9, 1.0], noise=3, noise_seed=5)]
    for kw in sets:
        a = synth.render_sequence(4, 32, 48, K, v, w, **kw)
        b = synth.render_sequence(4, 32, 48, K, v, w, mover=None, **kw)
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b)), kw
    clip = scases.smooth_clip(33, 70, 1, 21, t=1.0, shutter=0.0, samples=1, nsources=3)
    again = scases.smooth_clip(33, 70, 1, 21, t=1.0, shutter=0.0, samples=1, nsources=3)
    assert all(np.array_equal(x, y) for x, y in zip(clip["frames"], again["frames"]))
    mover = (5, 4, 9, 11, 7, 3)
    planes = synth.mover_planes(4, 32, 48, mover)
    assert planes.shape == (4, 32, 48) and planes.dtype == bool and (planes.reshape(4, -1).sum(axis=1) == 99).all()
    assert planes[0, 5:14, 4:15].all() and planes[3, 14:23, 25:36].all()
    plain, flow, mask = synth.render_sequence(4, 32, 48, K, v, w)
    moved, flow2, mask2 = synth.render_sequence(4, 32, 48, K, v, w, mover=mover)
    pair = synth.render_occluded_pair(32, 48, K, v, w, block=mover[:4], block_motion=(7, 3))
    block = pair[0][5:14, 4:15]
    assert np.array_equal(flow, flow2) and np.array_equal(mask, mask2)
    for j in range(4):
        assert np.array_equal(moved[j][planes[j]].reshape(9, 11, 3), block) and np.array_equal(moved[j][~planes[j]], plain[j][~planes[j]])
    assert np.array_equal(moved[1][8:17, 11:22], pair[1][8:17, 11:22])
    noisy = synth.render_sequence(4, 32, 48, K, v, w, mover=mover, noise=4)[0]  # the noise comes after the block
    assert np.abs(noisy.astype(np.int64) - moved).max() <= 4 and (noisy != moved).any()
    for bad in ((5, 4, 9, 11, 12, 3), (-1, 4, 9, 11, 0, 0), (5, 4, 0, 11, 0, 0), (5, 4, 9, 11, 0, 7), (5, 40, 9, 11, -14, 0)):
        with pytest.raises(ValueError):
            synth.render_sequence(4, 32, 48, K, v, w, mover=bad)
