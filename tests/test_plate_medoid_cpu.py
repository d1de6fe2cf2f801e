"""GPU-free tests of the colour-consistent plate (include/rsdsfm_plate_medoid.h): the definition (tests/plate_medoid_spec_numpy.py) against hand
answers, its three consequences -- with one channel it IS the lower median, with grey BGR candidates too, with two candidates the smaller packed
colour --, membership (a plate pixel is one of its candidates), the order of the layers, what the feature is for on the scene with a mover (bounds
derived, not measured), its golden fixture, the exported symbols and the launch count.  (The calls' refusals and the knob need a context:
tests/test_gpu_plate_medoid.py.)"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import denoise_spec_numpy as denoise  # noqa: E402
import plate_cases as cases  # noqa: E402
import plate_medoid_cases as mcases  # noqa: E402
import plate_medoid_spec_numpy as spec  # noqa: E402
import plate_spec_numpy as median_spec  # noqa: E402
from make_golden_plate import digest, median_cases  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_plate_medoid_v1.npz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_plate_medoid.h")).read()  # what this file tests is declared there
NEW_SYMBOLS = {"rsdsfm_plate_medoid_dev", "rsdsfm_plate_medoid_launches", "rsdsfm_set_plate_estimator"}
PLANES = ("image", "mask", "votes", "moving")


def _same(got, want, name=""):
    for k in PLANES:
        assert np.array_equal(got[k], want[k]), (name, k)
    assert list(got["counts"]) == list(want["counts"]), (name, got["counts"], want["counts"])


# ---------------------------------------------------------------------------------------------------
# hand answers
# ---------------------------------------------------------------------------------------------------
def test_the_triple_without_a_majority_is_a_candidate_and_the_median_is_not():
    case = mcases.no_majority()
    got = mcases.spec_of(case)
    assert (got["image"] == np.array(mcases.GREY, dtype=np.uint8)).all()  # costs 710 against 865 and 865
    assert (cases.spec_of(case)["image"] == np.array(mcases.PURPLE, dtype=np.uint8)).all()  # what the per-channel median makes of it
    assert mcases.PURPLE not in (mcases.GREY, mcases.RED, mcases.BLUE)
    # whichever of the three is the own frame, and with the own frame absent
    px = lambda c: np.broadcast_to(np.array(c, dtype=np.uint8), (4, 6, 3)).copy()
    full, none = np.ones((4, 6), dtype=np.uint8), np.zeros((4, 6), dtype=np.uint8)
    for order in ((mcases.RED, mcases.GREY, mcases.BLUE), (mcases.BLUE, mcases.RED, mcases.GREY)):
        assert (spec.medoid(px(order[0]), full, [(px(order[1]), full), (px(order[2]), full)])["image"] == np.array(mcases.GREY, dtype=np.uint8)).all()
    got = spec.medoid(px((1, 2, 3)), none, [(px(c), full) for c in (mcases.RED, mcases.GREY, mcases.BLUE)])
    assert (got["image"] == np.array(mcases.GREY, dtype=np.uint8)).all() and (got["moving"] == 0).all() and (got["votes"] == 3).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_constructed_cases_have_their_known_answers(channels):
    """all candidates equal; one outlier among fourteen equal candidates at layer positions 0, 6 and 13; the own frame as the outlier (the plate is
    the others' value, the flag 2 everywhere); two candidates (the smaller packed colour); an empty own mask; min_votes 15; the impulses"""
    names = set()
    for case in mcases.constructed(channels):
        got = mcases.spec_of(case)
        for k, want in case["want"].items():
            assert np.array_equal(np.asarray(got[k]), np.asarray(want)), (case["name"], k)
        assert sum(got["counts"]) == case["rmask"].size
        names.add(case["name"])
    assert {"all-equal", "one-outlier-at-0", "one-outlier-at-6", "one-outlier-at-13", "own-outlier", "two-candidates", "own-mask-empty", "min-votes-15"} <= names
    by_name = {c["name"]: c for c in mcases.constructed(channels)}
    assert (by_name["own-outlier"]["want"]["moving"] == 2).all() and by_name["min-votes-15"]["min_votes"] == 15


def test_two_candidates_give_the_smaller_packed_colour_not_the_channel_minimum():
    """consequence (c): (200, 1, 0) packs to 456 and (0, 0, 1) to 65536 -- the plate is (200, 1, 0), the per-channel minimum (0, 0, 0) is neither"""
    px = lambda c: np.broadcast_to(np.array(c, dtype=np.uint8), (3, 5, 3)).copy()
    full = np.ones((3, 5), dtype=np.uint8)
    a, b = (200, 1, 0), (0, 0, 1)
    for first, second in ((a, b), (b, a)):
        got = spec.medoid(px(first), full, [(px(second), full)], min_votes=2)
        assert (got["image"] == np.array(a, dtype=np.uint8)).all() and (got["votes"] == 2).all()
        assert (median_spec.median(px(first), full, [(px(second), full)], min_votes=2)["image"] == 0).all()
    case = {c["name"]: c for c in mcases.constructed(3)}["two-candidates"]
    assert not np.array_equal(case["want"]["image"], np.minimum(case["ref"], case["layers"][0][0]))  # the case can tell the two apart


# ---------------------------------------------------------------------------------------------------
# the consequences
# ---------------------------------------------------------------------------------------------------
def test_with_one_channel_the_medoid_is_the_lower_median():
    """consequence (a): every plane and the counts, at every shape and layer count of the median's own tests (the five records in turn, the
    parameters that change with the case) and on 300 gray cases of the seeded campaign"""
    for shape in cases.ACC_SHAPES:
        for L in cases.LAYER_COUNTS:
            ref, rmask, ls = cases.median_inputs(shape, 1, L)
            recs = list(cases.layer_records(1, L, phase=shape[1]))
            threshold, min_votes = cases.median_parameters(shape, L)
            _same(spec.medoid(ref, rmask, ls, recs, threshold=threshold, min_votes=min_votes), median_spec.median(ref, rmask, ls, recs, threshold=threshold, min_votes=min_votes),
                  (shape, L))
    layer_counts = set()
    for k, case in enumerate(mcases.random_cases(20240, 300, 1)):
        _same(mcases.spec_of(case), cases.spec_of(case), k)
        layer_counts.add(len(case["layers"]))
    assert layer_counts == set(range(15))


def test_grey_bgr_candidates_without_a_gain_give_the_medians_bytes():
    """consequence (b): b = g = r in every candidate and no record: the distance is 3 |x_i - x_j|"""
    grey = lambda a: np.repeat(np.asarray(a)[..., None], 3, axis=-1)
    for shape, L in (((5, 5), 3), ((17, 65), 7), ((37, 67), 14), ((16, 64), 0), ((15, 63), 4), ((3, 7), 1)):
        ref, rmask, ls = cases.median_inputs(shape, 1, L)
        bgr = [(grey(i), m) for i, m in ls]
        threshold, min_votes = cases.median_parameters(shape, L)
        got = spec.medoid(grey(ref), rmask, bgr, None, threshold=threshold, min_votes=min_votes)
        _same(got, median_spec.median(grey(ref), rmask, bgr, None, threshold=threshold, min_votes=min_votes), (shape, L))
        assert np.array_equal(got["image"], grey(median_spec.median(ref, rmask, ls, None, threshold=threshold, min_votes=min_votes)["image"]))


def test_every_plate_pixel_is_one_of_its_candidates():
    """300 seeded BGR cases: a set plate pixel equals the gained colour of one of its valid candidates, whole; the per-channel median does not
    (the campaign would notice a definition that mixed channels)"""
    mixed = 0
    for k, case in enumerate(mcases.random_cases(515, 300, 3)):
        got = mcases.spec_of(case)
        values, valid = spec.candidates(case["ref"], case["rmask"], case["layers"], None if case["records"] is None else list(case["records"]),
                                        case["min_overlap"] or spec.MIN_OVERLAP_DEFAULT, case["gain_mode"])
        member = lambda image: ((values == image.astype(np.int64)[None]).all(axis=-1) & valid).any(axis=0)
        on = got["mask"] != 0
        assert np.array_equal(on, valid.any(axis=0)) and member(got["image"])[on].all(), k
        assert (got["image"][~on] == 0).all() and np.array_equal(got["votes"], valid.sum(axis=0))
        mixed += int((~member(cases.spec_of(case)["image"]))[on].sum())
    assert mixed > 0


@pytest.mark.parametrize("channels", [1, 3])
def test_the_result_does_not_depend_on_the_order_of_the_layers(channels):
    ref, rmask, ls = cases.median_inputs((37, 67), channels, 5)
    recs = cases.layer_records(channels, 5)
    case = dict(ref=ref, rmask=rmask, layers=ls, records=recs, min_overlap=0, gain_mode=0, threshold=30, min_votes=3)
    want = mcases.spec_of(case)
    assert min(want["counts"][:3]) > 0
    rng = np.random.default_rng(5)
    for _ in range(8):
        perm = rng.permutation(5)
        _same(mcases.spec_of(mcases.shuffled(case, perm)), want, perm.tolist())
    for k, case in enumerate(mcases.random_cases(99, 40, channels)):
        perm = rng.permutation(len(case["layers"]))
        _same(mcases.spec_of(mcases.shuffled(case, perm)), mcases.spec_of(case), k)


# ---------------------------------------------------------------------------------------------------
# what the feature is for
# ---------------------------------------------------------------------------------------------------
def test_the_medoid_plate_removes_a_mover_and_the_flag_finds_it():
    """tests/test_plate_cpu.py's scene and bounds (five frames, noise +-6, no gain, threshold 12, a block of 255 in every frame, the five footprints
    disjoint in frame q's camera), derived for a medoid.  At an inspected pixel at most one candidate is a footprint's 255 (the footprints are
    disjoint) and m >= 2 are background, each channel within 6 of the clean byte c <= 223.  Two background candidates differ by at most 12 per
    channel, 36 in all; a background candidate i and the 255 differ by d_i >= 3 (255 - 229) = 78.  cost(255) = sum_j d_j, cost(i) <= 36 (m - 1) +
    d_i, so cost(255) - cost(i) >= sum_{j != i} (d_j - 36) >= 42 (m - 1) > 0: the medoid is a background candidate -- a strict majority of
    background candidates within +-6 outvotes the candidate at 255.  Hence
    (a) on the own frame's footprint and wherever all five sources see, |plate - clean| <= 6 per channel;
    (b) a pixel whose whole 3 x 3 window lies in the own footprint is moving: e >= CH (255 - 223 - 6) = 26 CH > 12 CH per pixel;
    (c) a pixel all five see whose 3 x 3 window touches no footprint is static: the plate is a candidate within 6 of the clean byte, as the own
        pixel is: they differ by at most 12 per channel, which is not > 12."""
    case, prints = cases.mover_scene()
    q, noise = case["q"], cases.MOVER_NOISE
    r = spec.run_spec(case)
    clean = case["clean"][q].astype(np.int64)
    rows, cols = prints.shape[1:]
    assert r["sources"] == [2, 1, 3, 0, 4] and clean.max() <= 223 and clean.min() >= 32 and case["threshold"] == 12
    planes = [r["ref"][:2]] + r["layers"]
    seen = np.stack([m != 0 for _, m in planes])
    ordered = prints[r["sources"]]
    for (image, mask), foot in zip(planes, ordered):  # the scene meets the conditions: every candidate is a footprint's 255 or within the noise
        on = mask != 0
        assert np.array_equal((image == 255).all(axis=-1) & on, foot)
        assert (np.abs(image.astype(np.int64) - clean)[on & ~foot] <= noise).all()
    any_print = prints.any(axis=0)
    assert prints.sum(axis=0).max() == 1  # pairwise disjoint: at most one candidate at 255
    own = ordered[0]
    all_five = seen.all(axis=0)
    inspect = own | all_five
    background = (seen & ~ordered).sum(axis=0)
    assert (background[inspect] >= 2).all() and ((seen & ordered).sum(axis=0)[inspect] <= 1).all()  # m >= 2 against at most one
    # (a)
    assert (np.abs(r["image"].astype(np.int64) - clean)[inspect] <= noise).all() and (r["mask"][inspect] == 1).all()
    # (b)
    interior = denoise.box3(own.astype(np.int64)) == 9
    assert interior.sum() == (cases.MOVER_HEIGHT - 2) * (cases.MOVER_WIDTH - 2) and (r["moving"][interior] == 2).all()
    # (c)
    quiet = all_five & (denoise.box3(any_print.astype(np.int64)) == 0)
    assert (r["moving"][quiet] == 1).all()
    assert inspect.sum() >= interior.sum() and quiet.sum() >= interior.sum() and quiet.sum() > rows * cols // 4  # a mask bug cannot empty the test
    assert (np.abs(r["image"].astype(np.int64) - r["ref"][0])[own] >= 26).all()  # the own frame itself still shows the block
    # and every plate pixel is a whole candidate
    values, valid = spec.candidates(r["ref"][0], r["ref"][1], r["layers"], None, gain_mode=1)
    assert ((values == r["image"].astype(np.int64)[None]).all(axis=-1) & valid).any(axis=0)[r["mask"] != 0].all()


# ---------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------
def test_spec_equals_the_golden_fixture(oracle):
    g = np.load(GOLDEN)
    plain = np.load(os.path.join(ROOT, "tests", "golden", "golden_plate_v1.npz"))
    all_cases = cases.all_cases(oracle.pose_table)
    medians = median_cases()
    assert {k.split("/")[0] for k in g.files} == {c["name"] for c in all_cases} | set(medians) and set(g.files) == set(plain.files)
    seen = np.zeros(4, dtype=np.int64)
    differ = 0
    for case in all_cases:
        n = case["name"] + "/"
        assert digest(case) == int(g[n + "digest"]), n
        r = spec.run_spec(case)
        for k in PLANES + ("records",):
            assert np.array_equal(r[k], g[n + k]), (n, k)
        assert list(r["counts"]) == g[n + "counts"].tolist() and sum(r["counts"]) == r["mask"].size, n
        assert all(np.array_equal(g[n + k], plain[n + k]) for k in ("mask", "votes", "records"))  # the renders, the mask and the votes are the median's
        if case["frames"][0].ndim == 2:
            assert all(np.array_equal(g[n + k], plain[n + k]) for k in PLANES + ("counts",)), n  # gray: the median's bytes
        else:
            differ += int((g[n + "image"] != plain[n + "image"]).sum())
        seen += np.array(r["counts"])
    for name, case in medians.items():
        r = mcases.spec_of(case)
        for k in PLANES:
            assert np.array_equal(r[k], g[name + "/" + k]), (name, k)
        assert list(r["counts"]) == g[name + "/counts"].tolist(), name
    assert (seen > 0).all() and differ > 0
    assert os.path.getsize(GOLDEN) <= 256 * 1024


# ---------------------------------------------------------------------------------------------------
# the host functions
# ---------------------------------------------------------------------------------------------------
def test_symbols_and_launch_counts(rsdsfm):
    assert NEW_SYMBOLS == set(rsdsfm.plate_medoid_declared_symbols()) and NEW_SYMBOLS <= set(rsdsfm.declared_symbols())
    for arith in ("reference", "fused"):
        lib = rsdsfm.load_library(arith=arith)
        assert all(hasattr(lib, n) for n in NEW_SYMBOLS)
        assert lib.rsdsfm_plate_medoid_launches() == 1
        assert lib.rsdsfm_set_plate_estimator(None, 1) == -1  # no context: RSDSFM_ERR_INVALID
    assert rsdsfm.plate_medoid_launches() == 1 == rsdsfm.plate_median_launches()
    assert (rsdsfm.PLATE_MEDIAN, rsdsfm.PLATE_MEDOID) == (0, 1)
    assert "NOT here" in HEADER_TEXT and "RSDSFM_PLATE_MEDIAN 0" in HEADER_TEXT and "RSDSFM_PLATE_MEDOID 1" in HEADER_TEXT
    for name in ("plate_medoid_dev", "plate_medoid", "set_plate_estimator", "plate_estimator"):
        assert hasattr(rsdsfm.Solver, name), name


def test_evaluate_refuses_a_plate_estimator_without_a_plate(rsdsfm):
    ev = rsdsfm.evaluate.evaluate_real_sequence
    frames = np.zeros((3, 8, 8), dtype=np.uint8)
    with pytest.raises(ValueError):
        ev(None, frames, plate_estimator="medoid")
    with pytest.raises(ValueError):
        ev(None, frames, stabilize=True, plate=1, plate_estimator="mean")
