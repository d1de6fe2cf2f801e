"""CPU: the generator of the temporal stages' campaign (tests/temporal_fuzz_cases.py; tests/fuzz_temporal.py runs it on the GPU) held to what it
promises -- records that depend on (n, seed) alone, the first 240 cases of seed 1 covering every family, channel count, side residue, chain
length, placement and strip (and its first 1200 records every layer count of the plate and every listed weight of the merge: one family of
twelve needs that many draws for fifteen values), every case's definition running and well defined, at most one case in four per call whose
definition's own output a kernel that does nothing would also give, nine wrong variants of the definitions each told apart by at least three
cases of the slice tests/test_gpu_temporal_fuzz.py runs, and the time that slice's definitions take here."""
import contextlib
import inspect
import time
import types

import numpy as np
import pytest

import denoise_spec_numpy as denoise_spec
import plate_spec_numpy as plate_spec
import retime_spec_numpy as retime_spec
import shutter_spec_numpy as shutter_spec
import stage_fuzz_cases as G
import superres_spec_numpy as superres_spec
import temporal_fuzz_cases as T
from test_gpu_temporal_fuzz import SLICE, SLICE_SEED
from test_stage_fuzz_cpu import SLICE_SECONDS, TRIVIAL_SHARE

COVERED = 240
RECORDS = 1200  # records alone are cheap: the plate's fifteen layer counts, one family of twelve, need this many draws of seed 1 to all occur
CAUGHT = 3  # cases of the slice that must tell a mutant from the definition


@pytest.fixture(scope="module")
def solved(oracle):
    """(case, inputs, the definition's outputs) of the first COVERED cases of seed 1, computed once; nobody modifies them.  The slice's
    definitions took 1.7 s on one CPU core when this was measured (and with the GPU's side 4.0 s on the MI355X's host) (SLICE_SECONDS, the sibling's bound for "a few seconds", is 6)"""
    out, seconds = [], 0.0
    for n in range(COVERED):
        t0 = time.perf_counter()
        case = T.random_case(n, SLICE_SEED)
        inp = T.inputs(case, oracle.pose_table)
        out.append((case, inp, T.expected(case, inp)))
        if n < SLICE:
            seconds += time.perf_counter() - t0
    return out, seconds


def test_records_depend_on_case_and_seed_alone():
    a = [T.random_case(n, s) for s in (1, 2) for n in range(400)]
    T.random_case(5, 9)  # (another draw in between changes nothing)
    b = [T.random_case(n, s) for s in (1, 2) for n in range(400)]
    assert a == b and all(repr(x) == repr(y) for x, y in zip(a, b))
    assert sum((a[n].family, a[n].rows, a[n].cols) != (a[400 + n].family, a[400 + n].rows, a[400 + n].cols) for n in range(400)) > 390  # two campaigns
    for c in a:
        assert c.family in T.FAMILIES + ("stage",) and min(c.rows, c.cols) >= 2
        if c.family == "stage":  # the existing campaign's own record, untouched
            assert c.stage == G.random_case(c.n, c.seed) and (c.rows, c.cols) == (c.stage.rows, c.stage.cols)
            continue
        assert c.channels in (1, 3) and set(c.place["planes"]) <= set(T.PLANE_OFFSETS) and set(c.place["cells"]) <= set(T.CELL_OFFSETS)
        scale = c.params.get("scale", 1)
        if c.family in T.PRIMITIVES:
            assert c.rows * c.cols * (scale * scale if c.family == "superres_render" else 1) <= G.MAX_PIXELS
            assert (max(c.rows, c.cols) in G.STRIP_LONG and min(c.rows, c.cols) <= 8) if c.strip else max(c.rows, c.cols) <= 300
        else:
            assert c.rows <= T.FRAME_ROWS and c.cols <= T.FRAME_COLS and not c.strip
    assert 0.2 < sum(c.family == "stage" for c in a) / len(a) < 0.3  # about one case in four


def test_the_first_cases_cover_every_family_and_edge():
    cases = [T.random_case(n, SLICE_SEED) for n in range(COVERED)]
    mine = [c for c in cases if c.family != "stage"]
    assert [c.family for c in mine[:len(T.FAMILIES)]] != list(T.FAMILIES)  # drawn, not dealt in turn
    for family in T.FAMILIES:
        of = [c for c in mine if c.family == family]
        assert len(of) >= 8 and {c.channels for c in of} == {1, 3}, family
    assert {c.cols % 4 for c in mine} == {0, 1, 2, 3} and {(c.rows * c.cols) % 2 for c in mine} == {0, 1}
    tiled = [c for c in mine if c.family in T.TILE]
    assert {0, 1, 63} <= {c.cols % 64 for c in tiled} and {0, 1, 15} <= {c.rows % 16 for c in tiled}
    for family in T.TILE:
        of = [c for c in mine if c.family == family]
        assert any(c.rows > 16 and c.cols > 64 and c.rows % 16 and c.cols % 64 for c in of), family  # several ragged tiles both ways
        assert any(c.strip and c.cols > c.rows for c in of), family  # 16 tiles and more across
    plates = {c.params["L"] for c in mine if c.family == "plate"}
    assert len(plates) >= 8 and {0, 14} & plates and any(L not in (0, 2, 4, 7, 14) for L in plates)  # counts between the kernel's instances ...
    more = [T.random_case(n, SLICE_SEED) for n in range(RECORDS)]
    assert {c.params["L"] for c in more if c.family == "plate"} == set(range(15))  # ... and every one of them within the first RECORDS
    for family, key in (("shutter", "S"), ("denoise", "L"), ("superres_accumulate", "L")):
        lengths = {min(c.params[key], 3) for c in mine if c.family == family}
        assert {1, 2, 3} <= lengths, (family, lengths)
    assert {c.params["scale"] for c in mine if c.family == "superres_frame"} == {1, 2, 3, 4} == {c.params["scale"] for c in mine if c.family == "superres_render"}
    assert {c.params["nsrc"] for c in mine if c.family == "retime_frame"} == {1, 2}
    for family in ("denoise_frame", "superres_frame", "plate_frame"):
        nsrc = {c.params["nsrc"] for c in mine if c.family == family}
        assert min(nsrc) <= 2 and max(nsrc) >= 13 and len(nsrc) >= 6, (family, nsrc)
    assert {c.params["nsrc"] for c in mine if c.family in ("denoise_frame", "superres_frame", "plate_frame")} == set(range(1, 16))
    assert {(c.params["occlusion"], c.params["search"]) for c in mine if c.family in T.FRAMES} == {(0, 0), (1, 0), (1, 1)}
    assert {o for c in mine for o in c.place["planes"]} == set(T.PLANE_OFFSETS) and {o for c in mine for o in c.place["cells"]} == set(T.CELL_OFFSETS)
    for family in T.PRIMITIVES:  # ... and the first plane and the first cell of every primitive family at every residue
        of = [c for c in mine if c.family == family]
        assert {c.place["planes"][0] for c in of} == set(T.PLANE_OFFSETS) and {c.place["cells"][0] for c in of} == set(T.CELL_OFFSETS), family
    strips = [c for c in mine if c.strip]
    assert any(c.rows > c.cols for c in strips) and any(c.cols > c.rows for c in strips)  # strips run both ways
    merges = [c.params for c in mine if c.family == "merge"]
    assert any(not p["b"] for p in merges) and {"empty", "full"} <= {k for p in merges for k in p["masks"]}
    assert {0, 1, 32768, 32769, 65535, T.WEIGHT_REFUSED} <= {c.params["weight"] for c in more if c.family == "merge"}  # (within the first RECORDS)


def test_every_definition_runs_and_is_well_defined(solved):
    for case, inp, want in solved[0]:
        assert T.undefined(case, inp, want) == [], T.describe(case)


def test_the_campaign_does_not_pass_by_testing_nothing(solved):
    """per call, at most one case in four whose definition's own output says nothing: a merge with no set pixel (or the refused weight), a
    chain or a frame that averages nothing, a plate with no votes, a render with an empty proximity plane, a record over no pixel -- and the
    existing campaign's own calls, as tests/test_stage_fuzz_cpu.py counts them"""
    total, empty = {}, {}
    for case, inp, want in solved[0]:
        for what, says_nothing in T.trivial(case, inp, want).items():
            total[what] = total.get(what, 0) + 1
            empty[what] = empty.get(what, 0) + bool(says_nothing)
    print({k: "%d of %d" % (empty[k], total[k]) for k in sorted(total)})
    assert set(T.FAMILIES) <= set(total)
    for what in T.FAMILIES:
        assert empty[what] <= TRIVIAL_SHARE * total[what], (what, empty[what], total[what])


# ---------------------------------------------------------------------------------------------------
# mutants: wrong variants of the definitions that the slice's inputs must tell from the right ones
# ---------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _mutant(*edits, aliases=()):
    """edits: (module, old text, new text), the module's functions recompiled from its source with the one replacement and put in its place;
    aliases: (module, name, getter), the getter's value set after the edits.  Everything is put back on exit"""
    saved = []
    try:
        for module, old, new in edits:
            src = inspect.getsource(module)
            assert src.count(old) == 1, (module.__name__, old)
            ns = dict(module.__dict__)
            exec(compile(src.replace(old, new), module.__file__, "exec"), ns)
            for k, v in ns.items():
                if isinstance(v, types.FunctionType) and v.__globals__ is ns:
                    saved.append((module, k, getattr(module, k)))
                    setattr(module, k, v)
        for module, name, value in aliases:
            saved.append((module, name, getattr(module, name)))
            setattr(module, name, value())
        yield
    finally:
        for module, k, v in reversed(saved):
            setattr(module, k, v)


def _tiled_box3(a):
    """the 3 x 3 sums taken per 16 x 64 tile with a zero halo: what a kernel that forgot the halo computes"""
    box3, out = _BOX3, np.zeros_like(a)
    for y0 in range(0, a.shape[0], 16):
        for x0 in range(0, a.shape[1], 64):
            out[y0:y0 + 16, x0:x0 + 64] = box3(a[y0:y0 + 16, x0:x0 + 64])
    return out


_BOX3 = denoise_spec.box3
_ROUND = "(2 * s + n[..., None]) // den[..., None]"
_FLOOR = "(2 * s) // den[..., None]"


def _mutants():
    tiled = dict(aliases=((denoise_spec, "box3", lambda: _tiled_box3), (superres_spec, "box3", lambda: _tiled_box3)))
    no_round = ((denoise_spec, "(int(G[c]) * lay[..., c] + 32768) >> 16", "(int(G[c]) * lay[..., c]) >> 16"),)
    return [
        ("a: the denoise's box3 per tile, zero halo", ("denoise", "denoise_frame"), (), tiled),
        ("b: the same on the super-resolution's fine grid", ("superres_accumulate", "superres_frame"), (), tiled),
        ("c: the same for the plate's flag", ("plate", "plate_frame"), (), tiled),
        ("d: the resolves floor", T.CHAINS + ("shutter_frame", "denoise_frame", "superres_frame"),
         ((shutter_spec, _ROUND, _FLOOR), (denoise_spec, _ROUND, _FLOOR), (superres_spec, _ROUND, _FLOOR)), {}),
        ("e: the gain without its + 32768", ("denoise", "superres_accumulate", "plate", "denoise_frame", "superres_frame", "plate_frame"), no_round,
         dict(aliases=((superres_spec, "gained", lambda: denoise_spec.gained),))),
        ("f: the upper median", ("plate", "plate_frame"), ((plate_spec, "index = np.maximum(n - 1, 0) >> 1", "index = n >> 1"),), {}),
        ("g: the merge's threshold strict", ("merge", "retime_frame"),
         ((retime_spec, "source[both & (d <= threshold)] = DISSOLVED\n    source[both & (d > threshold)]", "source[both & (d < threshold)] = DISSOLVED\n    source[both & (d >= threshold)]"),), {}),
        ("h: min_samples compared with >", ("shutter", "shutter_frame"), ((shutter_spec, "ok = n >= min_samples", "ok = n > min_samples"),), {}),
        ("i: u without its + 8", ("superres_accumulate", "superres_frame"), ((superres_spec, ".astype(np.int64) + 8) >> 4", ".astype(np.int64)) >> 4"),), {}),
    ]


def _same_outputs(a, b):
    for k in a:
        if isinstance(a[k], np.ndarray) and not np.array_equal(a[k], b[k]):
            return False
        if k == "counts" and list(a[k]) != list(b[k]):
            return False
    return a.get("cells_before") is None or np.array_equal(a["cells_before"], b["cells_before"])


@pytest.mark.parametrize("mutant", _mutants(), ids=lambda m: m[0][0])
def test_the_slice_tells_the_mutant_from_the_definition(solved, mutant):
    name, families, edits, kw = mutant
    mine = [(case, inp, want) for case, inp, want in solved[0][:SLICE] if case.family in families and not want.get("refused")]
    with _mutant(*edits, **kw):
        caught = [case.n for case, inp, want in mine if not _same_outputs(want, T.expected(case, inp))]
    print(name, "caught by", len(caught), "of", len(mine), "cases:", caught)
    for case, inp, want in mine[:3]:  # ... and put back: the definitions are themselves again
        assert _same_outputs(want, T.expected(case, inp))
    if name[0] in "abc":  # per family: each of the three kernels has its own halo
        assert len([n for n in caught if solved[0][n][0].family == families[0]]) >= 1, name
    assert len(caught) >= CAUGHT, (name, caught)


def test_the_tiled_mutant_shows_only_across_a_tile_border():
    """the condition on the generator: the tiled box3 changes bytes at every shape that crosses a tile border and at none that does not"""
    import denoise_cases as dcases

    for shape, crosses in (((16, 64), False), ((5, 5), False), ((17, 64), True), ((16, 65), True), ((37, 67), True)):
        ref, rmask = dcases.reference(*shape, 3)
        layers = dcases.layers(ref, *shape, 3, 2)
        want = denoise_spec.denoise(ref, rmask, layers, None, strength=40)
        with _mutant(aliases=((denoise_spec, "box3", lambda: _tiled_box3),)):
            got = denoise_spec.denoise(ref, rmask, layers, None, strength=40)
        assert _same_outputs(want, got) != crosses, shape


def test_the_slices_definitions_take_seconds(solved):
    print("the definitions of the slice's %d cases took %.2f s" % (SLICE, solved[1]))
    assert solved[1] < SLICE_SECONDS
