"""CPU: the generator of the stages' campaign (tests/stage_fuzz_cases.py; tests/fuzz_stages.py runs it on the GPU) held to what it promises --
records that depend on (n, seed) alone, the first 240 cases of seed 1 covering every family, channel count, side residue, portrait frame and
strip, every case's definition running and well defined, at most one case in four per call whose definition's own output a kernel that does
nothing would also give, the definitions against the second formulations the tree has on the small cases, the edges the slice of
tests/test_gpu_stage_fuzz.py has to reach, and the time that slice's definitions take here."""
import time

import numpy as np
import pytest

import stabilize_blend_cases as blend_cases
import stabilize_crop_spec_numpy as crop_spec
import stabilize_inpaint_cases as inpaint_cases
import stage_fuzz_cases as G
from test_gpu_stage_fuzz import SLICE, SLICE_SEED
from test_stabilize_crop_cpu import _brute_window

COVERED = 240
TRIVIAL_SHARE = 0.25
# measured: the definitions of the slice's 120 cases take 1.9 s on one CPU core (and with the GPU's side 3.1 s on the MI355X's host); the
# bound is "a few seconds", with room for a slower machine
SLICE_SECONDS = 6.0


@pytest.fixture(scope="module")
def solved(oracle):
    """(case, inputs, the definition's outputs) of the first COVERED cases of seed 1, computed once; nobody modifies them"""
    out, seconds = [], 0.0
    for n in range(COVERED):
        t0 = time.perf_counter()
        case = G.random_case(n, SLICE_SEED)
        inp = G.inputs(case, oracle.pose_table)
        out.append((case, inp, G.expected(case, inp)))
        if n < SLICE:
            seconds += time.perf_counter() - t0
    return out, seconds


def test_records_depend_on_case_and_seed_alone():
    a = [G.random_case(n, s) for s in (1, 2) for n in range(400)]
    G.random_case(5, 9)  # (another draw in between changes nothing)
    b = [G.random_case(n, s) for s in (1, 2) for n in range(400)]
    assert a == b and all(repr(x) == repr(y) for x, y in zip(a, b))
    differ = sum(a[n] != a[400 + n] and (a[n].family, a[n].rows, a[n].cols) != (a[400 + n].family, a[400 + n].rows, a[400 + n].cols) for n in range(400))
    assert differ > 390  # seeds 1 and 2 are different campaigns
    for c in a:
        assert c.family in G.FAMILIES and c.rows * c.cols <= G.MAX_PIXELS and min(c.rows, c.cols) >= 2
        assert (max(c.rows, c.cols) in G.STRIP_LONG and min(c.rows, c.cols) <= 8) if c.strip else max(c.rows, c.cols) <= 300
        assert (c.channels in (1, 3)) == (c.family in G.WITH_CHANNELS)
    assert 0.09 < sum(c.strip for c in a) / len(a) < 0.18  # one case in about ten (0.137 by the shares)


def test_the_first_cases_cover_every_family_and_edge():
    cases = [G.random_case(n, SLICE_SEED) for n in range(COVERED)]
    assert [c.family for c in cases[:len(G.FAMILIES)]] != list(G.FAMILIES)  # drawn, not dealt in turn
    for family in G.FAMILIES:
        mine = [c for c in cases if c.family == family]
        assert len(mine) >= 15, family
        if family in G.WITH_CHANNELS:
            assert {c.channels for c in mine} == {1, 3}, family
        sides = [s for c in mine for s in (c.rows, c.cols)]
        assert any(s % 4 for s in sides) and any(s % 64 == 0 for s in sides), family
        assert any(c.rows > c.cols and not c.strip for c in mine) and any(c.strip for c in mine), family
    strips = [c for c in cases if c.strip]
    assert any(c.rows > c.cols for c in strips) and any(c.cols > c.rows for c in strips)  # strips run both ways
    assert any((c.rows * c.cols) % 4 for c in cases) and any(c.rows % 16 and c.cols % 64 for c in cases)


def test_every_definition_runs_and_is_well_defined(solved):
    for case, inp, want in solved[0]:
        assert G.undefined(case, inp, want) == [], G.describe(case)


def test_the_campaign_does_not_pass_by_testing_nothing(solved):
    """per call, at most one case in four whose definition's own output says nothing: a link with n = 0, a fusion that fills no pixel, a
    fill or window pass that takes none, the window (0, 0, 0, 0), a layer that neither fills nor blends, an inpainting that writes nothing,
    a stabiliser's mask of one value, a flow check that keeps nothing or everything, a distance plane of one value"""
    total, empty = {}, {}
    for case, inp, want in solved[0]:
        for what, says_nothing in G.trivial(case, inp, want).items():
            total[what] = total.get(what, 0) + 1
            empty[what] = empty.get(what, 0) + bool(says_nothing)
    print({k: "%d of %d" % (empty[k], total[k]) for k in sorted(total)})
    assert set(total) == {"flow_check", "link", "fuse", "stabilize", "fill", "crop_window", "window_frame", "seam_distance", "blend", "inpaint"}
    for what in total:
        assert empty[what] <= TRIVIAL_SHARE * total[what], (what, empty[what], total[what])


def test_definitions_equal_their_second_formulations_on_the_small_cases(oracle):
    """the inpainting cell by cell in Python integers, the seam distance from its definition, the window by brute force: on the campaign's own
    cases of at most 400 pixels (the first 600 of seeds 1 and 2)"""
    seen = dict(inpaint=0, seam=0, crop=0)
    for seed in (1, 2):
        for n in range(600):
            case = G.random_case(n, seed)
            if case.family not in seen or case.rows * case.cols > 400:
                continue
            inp = G.inputs(case, oracle.pose_table)
            want = G.expected(case, inp)
            seen[case.family] += 1
            if case.family == "inpaint":
                image, source = inp["image"].copy(), np.zeros_like(inp["mask"])
                count = inpaint_cases.loop_inpaint(image, inp["mask"], source)
                assert count == want["count"] and np.array_equal(image, want["image"]) and np.array_equal(source, want["source"]), G.describe(case)
            elif case.family == "seam":
                mask = inp["mask"] if case.op == "distance" else inp["own"]
                assert np.array_equal(blend_cases.brute_distance(mask, case.params["feather"]), want["dist"]), G.describe(case)
            else:
                p = case.params
                margin = crop_spec.MARGIN_DEFAULT if p["margin"] is None else p["margin"]
                assert _brute_window(inp["masks"], p["max_empty"], margin) == want["found"], G.describe(case)
    assert min(seen.values()) >= 5, seen


def test_the_slice_reaches_the_edges_it_is_there_for(rsdsfm, solved):
    """among the slice's cases: a window search and a seam distance on rows longer than 1024 columns (the row scan's carry, the distance's row
    segments) with empties before column 1024 and fewer of them allowed than there are; a blended layer whose last pixels lie in the byte tail
    (rows * cols % 4 != 0) deep inside the own frame (distance = feather, source 1, layer set: the pixels a `<=` for the `<` would blend) and
    one with a feathered pixel there; an inpainting with holes to fill; pyramids on either side of the 8160-cell single-workgroup
    threshold; frames of several 64 x 16 tiles with ragged edges"""
    seen = set()
    for case, inp, want in solved[0][:SLICE]:
        rows, cols, p = case.rows, case.cols, case.params
        tail = (rows * cols) % 4
        if case.family == "crop" and cols > 1024:
            common = crop_spec.common_mask(inp["masks"])
            if (~common[:, :1024]).any() and p["max_empty"] < (~common).sum():  # a carry that is not 0, and a bound that some rectangle breaks
                seen.add("row scan carry")
        if case.family == "seam" and cols > 1024 and 0 < int((want["dist"] == 0).sum()) < rows * cols:
            seen.add("distance row segments")
        if case.op == "blend" and tail:
            last = slice(rows * cols - tail, rows * cols)
            flat = lambda a: a.reshape(-1)[last]
            live = (flat(inp["source"]) == 1) & (flat(inp["lmask"]) != 0)
            if (live & (flat(inp["dist"]) == p["feather"])).any():
                seen.add("byte tail deep inside")
            if (live & (flat(inp["dist"]) < p["feather"])).any():
                seen.add("byte tail feathered")
        if case.family == "inpaint" and 0 < want["count"] < rows * cols:
            seen.add("inpaint holes")
        if case.family in ("dense", "stabilize", "fill", "crop", "inpaint"):  # (3 launches: the single workgroup takes the pyramid from level 1)
            seen.add("pyramid of one workgroup" if rsdsfm.inpaint_launches(rows, cols) == 3 else "pyramid with large levels")
        if case.family in ("link", "fuse", "dense") and rows > 32 and cols > 128 and rows % 16 and cols % 64:
            seen.add("ragged tiles")
    assert seen == {"row scan carry", "distance row segments", "byte tail deep inside", "byte tail feathered", "inpaint holes", "pyramid of one workgroup",
                    "pyramid with large levels", "ragged tiles"}


def test_the_slices_definitions_take_seconds(solved):
    print("the definitions of the slice's %d cases took %.2f s" % (SLICE, solved[1]))
    assert solved[1] < SLICE_SECONDS


def test_planted_windows_equal_the_definition_at_a_tenth_of_the_size():
    """tests/test_gpu_stage_fuzz.py::test_window_search_past_one_grid's layout at (150, 150): the definition gives the planted rectangle, and
    the larger one in the top rows once it is there"""
    low, top = G.planted_window(150), G.planted_window(150, second=True)
    assert crop_spec.crop_window([G.planted_mask(150, [low])], 0, 0) == low
    assert crop_spec.crop_window([G.planted_mask(150, [low, top])], 0, 0) == top and top[2] > low[2]
    big_low, big_top = G.planted_window(1500), G.planted_window(1500, second=True)
    assert big_low[0] >= 1420 and big_low[0] + big_low[2] <= 1500 and big_low[0] * 1500 > 8192 * 256  # every admissible anchor is past the first grid
    assert (big_top[0] + big_top[2]) * 1500 < 8192 * 256 and big_top[2] > big_low[2]                   # ... and the second rectangle's within it
