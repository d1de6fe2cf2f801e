"""GPU-free tests of the multi-frame super-resolution (include/rsdsfm_superres.h): the definition (tests/superres_spec_numpy.py) against its
golden fixture, its identities (scale 1 is the crop stage's render, no layer, an unrelated layer, the order of the layers), the proximity at
its extremes, the largest sums, the quality on the aliased shift scene, the host functions' refusals, the exported symbols, the launch
counts and the kernels' metadata."""
import ctypes
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import stabilize_crop_spec_numpy as crop  # noqa: E402
import superres_cases as cases  # noqa: E402
import superres_spec_numpy as spec  # noqa: E402
from make_golden_superres import digest  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_superres_v1.npz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_superres.h")).read()  # what this file tests is declared there: without the header, nothing here runs
NEW_SYMBOLS = {"rsdsfm_superres_params_init", "rsdsfm_superres_render_dev", "rsdsfm_superres_render_launches", "rsdsfm_superres_accumulate_dev",
               "rsdsfm_superres_accumulate_launches", "rsdsfm_superres_frame_dev", "rsdsfm_superres_launches", "rsdsfm_superres_video_dev"}
ERR_INVALID = -1


# ---------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------
def test_spec_equals_the_golden_fixture(oracle):
    g = np.load(GOLDEN)
    all_cases = cases.all_cases(oracle.pose_table)
    assert {k.split("/")[0] for k in g.files} == {c["name"] for c in all_cases}
    seen = np.zeros(3, dtype=np.int64)
    for case in all_cases:
        n = case["name"] + "/"
        assert digest(case) == int(g[n + "digest"]), n
        r = cases.run_spec(case)
        for k in ("image", "mask", "weight", "records"):
            assert np.array_equal(r[k], g[n + k]), (n, k)
        rows, cols = case["depths"][0].shape
        assert r["mask"].shape == (case["scale"] * rows, case["scale"] * cols)
        assert list(r["counts"]) == g[n + "counts"].tolist() and sum(r["counts"]) == r["mask"].size, n
        assert np.array_equal(r["mask"], (r["planes"][0]["prox"] != 0).astype(np.uint8)), n  # set exactly where the own frame is valid
        seen += np.array(r["counts"])
    assert (seen > 0).all()
    assert os.path.getsize(GOLDEN) <= 256 * 1024
    assert {c["frames"][0].ndim for c in all_cases} == {2, 3} and {c["scale"] for c in all_cases} == {1, 2, 3, 4}
    assert {len(cases.sources_and_poses(c)[0]) for c in all_cases} >= {1, 2, 3, 5}
    assert not np.array_equal(g["gained/image"], g["gain-off/image"])
    assert 0 < g["fold-plain/counts"][1]  # parallax: some pixels keep the own frame alone


@pytest.mark.parametrize("kind", ["identity", "pose"])
@pytest.mark.parametrize("channels", [1, 3])
def test_scale_1_is_the_crop_stages_render(kind, channels):
    """bil and prox != 0 are stabilize_crop_spec_numpy.backward_warp_window's image and mask, for the full window and a zoomed one"""
    rows, cols = 13, 21
    s = cases.render_source(rows, cols, channels, kind)
    for window in ((0, 0, rows, cols), (2, 3, 8, (8 * cols) // rows)):
        r = spec.render(s["image"], s["depth"], s["R"], s["t"], s["K"], s["M"], s["m"], 1, window)
        want = crop.stabilize_frame_window(s["image"], s["depth"], s["R"], s["t"], s["K"], s["M"], s["m"], window)
        assert np.array_equal(r["bil"], want["image"]) and np.array_equal((r["prox"] != 0).astype(np.uint8), want["mask"]), window
        assert want["mask"].any() and ((r["prox"] == 0) | (r["prox"] <= 16)).all()
        keep = r["prox"] != 0
        assert not r["near"][~keep].any() and not r["bil"][~keep].any()
    if kind == "identity":  # the full window at scale 1 samples every source pixel itself: nearest == bilinear == the image, prox 16
        r = spec.render(s["image"], s["depth"], s["R"], s["t"], s["K"], s["M"], s["m"], 1)
        assert np.array_equal(r["near"], s["image"]) and np.array_equal(r["bil"], s["image"]) and (r["prox"] == 16).all()


def test_a_source_without_a_valid_depth_renders_nothing():
    s = cases.render_source(5, 9, 3, "empty")
    r = spec.render(s["image"], s["depth"], s["R"], s["t"], s["K"], s["M"], s["m"], 3)
    assert r["bil"].shape == (15, 27, 3) and not r["bil"].any() and not r["near"].any() and not r["prox"].any()


def test_the_targets_are_the_crop_specs_with_the_output_size():
    for S in (1, 2, 3, 4):
        tx, ty = spec.fine_targets((2, 3, 9, 14), 12, 20, S)
        iy, ix = np.mgrid[0:S * 12, 0:S * 20].astype(np.float64)
        assert np.array_equal(tx, (3.0 + (ix + 0.5) * (14.0 / (S * 20))) - 0.5) and np.array_equal(ty, (2.0 + (iy + 0.5) * (9.0 / (S * 12))) - 0.5)
    tx, ty = spec.fine_targets((0, 0, 12, 20), 12, 20, 1)
    cx, cy = crop.window_targets((0, 0, 12, 20), 12, 20)
    assert np.array_equal(tx, cx) and np.array_equal(ty, cy)


def test_prox_at_its_extremes():
    """a = 0 gives 16, a = 0.5 on either axis gives 1, and the a = 0.5 tie goes to i1"""
    z = np.zeros(1)
    assert spec.proximity(z, z).tolist() == [16] and spec.proximity(z + 0.5, z).tolist() == [1] and spec.proximity(z, z + 0.5).tolist() == [1]
    assert spec.proximity(z + 0.5, z + 0.5).tolist() == [1] and spec.proximity(z + 0.25, z + 0.25).tolist() == [4] and spec.proximity(z + 0.75, z + 0.25).tolist() == [4]
    a = np.linspace(0.0, 1.0, 4097)[:-1]
    q = spec.proximity(a[:, None], a[None, :])
    assert q.min() == 1 and q.max() == 16 and np.array_equal(q, q.T) and np.array_equal(q, spec.proximity(1.0 - a[:, None], a[None, :]))  # symmetric about 0.5
    image = np.arange(12, dtype=np.uint8).reshape(3, 4) * 10
    px, py = np.array([[0.0, 0.5, 1.49, 2.5, 3.0]]), np.array([[1.0, 0.5, 1.5, 0.25, 2.0]])
    bil, near, prox = spec.sample_planes(image, px, py, np.ones((1, 5), dtype=bool))
    assert near.tolist() == [[40, 50, 90, 30, 110]]  # (0, 1); tie -> (1, 1); (1, 2): a_y = 0.5 -> row 2, a_x = 0.49 -> col 1; tie -> col 3; the last sample
    assert prox.tolist() == [[16, 1, 1, 1, 16]] and bil[0, 0] == 40 and bil[0, 4] == 110
    _, near0, prox0 = spec.sample_planes(image, px, py, np.zeros((1, 5), dtype=bool))
    assert not near0.any() and not prox0.any()


# ---------------------------------------------------------------------------------------------------
# the accumulate
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
def test_no_layer_returns_the_reference(channels):
    ref, near, prox = cases.reference(17, 65, channels)
    r = spec.accumulate(ref, near, prox, [])
    on = prox != 0
    keep = on if channels == 1 else on[..., None]
    assert np.array_equal(r["image"], np.where(keep, ref, 0)) and np.array_equal(r["mask"], on.astype(np.uint8))
    assert np.array_equal(r["weight"], prox) and r["counts"] == [int((~on).sum()), int(on.sum()), 0]


@pytest.mark.parametrize("channels", [1, 3])
def test_an_unrelated_layer_leaves_the_reference(channels):
    """a layer that disagrees with the own frame everywhere has w = 0: R's bytes exactly (not the nearest samples), weight qR"""
    rows, cols = 16, 64
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    rng = np.random.default_rng(4)
    ref = rng.integers(0, 100, size=shape, dtype=np.uint8)
    near = rng.integers(0, 256, size=shape, dtype=np.uint8)
    layer = (ref.astype(np.int64) + rng.integers(60, 150, size=shape)).astype(np.uint8)
    prox = rng.integers(1, 17, size=(rows, cols)).astype(np.uint8)
    r = spec.accumulate(ref, near, prox, [(layer, layer, prox), (layer[::-1].copy() | 128, near, prox[::-1].copy())])
    assert np.array_equal(r["image"], ref) and np.array_equal(r["weight"], prox) and r["counts"] == [0, rows * cols, 0]


@pytest.mark.parametrize("channels", [1, 3])
def test_the_result_does_not_depend_on_the_order_of_three_layers(channels):
    ref, near, prox = cases.reference(37, 67, channels)
    ls = cases.layers(ref, 37, 67, channels, 3)
    recs = [cases.records(channels)[k] for k in ("plain", "low", "small")]
    want = spec.accumulate(ref, near, prox, ls, recs, strength=30)
    assert min(want["counts"]) > 0
    for perm in itertools.permutations(range(3)):
        got = spec.accumulate(ref, near, prox, [ls[i] for i in perm], [recs[i] for i in perm], strength=30)
        for k in ("image", "mask", "weight"):
            assert np.array_equal(got[k], want[k]), perm
        assert got["counts"] == want["counts"]


def test_the_weight_is_the_patch_weight_times_the_proximity():
    """u = (w qL + 8) >> 4: 16 at w = qL = 16, 0 at w = 0, and rounds half up; the merged pixel is the weighted mean of nearest samples"""
    full16 = np.full((5, 5), 16, dtype=np.uint8)
    ref = np.full((5, 5), 40, dtype=np.uint8)
    u, w = spec.weights(ref, full16, ref, full16, [65536])
    assert (u == 16).all() and (w == 16).all()
    for q, want in ((1, 1), (8, 8), (9, 9), (16, 16)):
        assert (spec.weights(ref, full16, ref, np.full((5, 5), q, dtype=np.uint8), [65536])[0] == want).all()
    far = np.full((5, 5), 200, dtype=np.uint8)
    assert not spec.weights(ref, full16, far, full16, [65536])[0].any()
    # w = 8 (D = 9 * 9 per 9 pixels at h = 18 -> 16 * 81 // (18 * 9) = 8) and qL = 3: (24 + 8) >> 4 = 2; qL = 1: (8 + 8) >> 4 = 1
    off = np.full((5, 5), 49, dtype=np.uint8)
    assert spec.weights(ref, full16, off, np.full((5, 5), 3, dtype=np.uint8), [65536], 18)[0][2, 2] == 2
    assert spec.weights(ref, full16, off, np.full((5, 5), 1, dtype=np.uint8), [65536], 18)[0][2, 2] == 1
    # own nearest 100 at prox 4, a layer's nearest 60 at u = 12 -> (4 * 100 + 12 * 60) / 16 = 70; the bilinear sample (40) does not show
    r = spec.accumulate(ref, np.full((5, 5), 100, dtype=np.uint8), np.full((5, 5), 4, dtype=np.uint8), [(ref, np.full((5, 5), 60, dtype=np.uint8), np.full((5, 5), 12, dtype=np.uint8))])
    assert (r["image"] == 70).all() and (r["weight"] == 16).all() and r["counts"] == [0, 0, 25]


def test_fourteen_saturated_layers_fit_the_cells():
    ref = np.full((4, 6, 3), 255, dtype=np.uint8)
    q = np.full((4, 6), 16, dtype=np.uint8)
    r = spec.accumulate(ref, ref, q, [(ref, ref, q)] * spec.LAYERS_MAX)
    last = r["cells"][-1]
    assert (last[..., 3] == 240).all() and (last[..., :3] == 61200).all() and last.dtype == np.uint16
    assert (r["image"] == 255).all() and (r["weight"] == 240).all() and r["counts"] == [0, 0, 24]
    assert spec.LAYERS_MAX == 2 * spec.RADIUS_MAX == 14 and spec.PROX_MAX * (1 + spec.LAYERS_MAX) * 255 < 65536
    with pytest.raises(AssertionError):
        spec.accumulate(ref, ref, q, [(ref, ref, q)] * 15)


# ---------------------------------------------------------------------------------------------------
# quality
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,bound", [(2, 0.85), (3, 0.95)])
def test_the_aliased_shift_scene_gains_detail(scale, bound):
    """five frames of the aliased shift scene (a fine texture of sigma 1 fine pixel seen through a scale x scale box sensor at displacements that
    cover every phase at scale 2, integer noise in [-6, 6]); over the fine pixels every source sees, the mean absolute error against the fine
    texture is at most 0.85 (scale 2) / 0.95 (scale 3) of the one-source call's, which is the bilinear upscale of the own frame.  Measured on
    the definition, seeds 0 .. 2: scale 2 BGR 0.658 - 0.664, gray 0.665 - 0.671; scale 3 BGR 0.792 - 0.798, gray 0.824 - 0.835"""
    for channels in (3, 1):
        ratios = []
        for seed in range(3):
            case = cases.shift_clip(scale, channels, seed)
            ratio, r = cases.quality_ratio(case)
            assert (r["mask"] == 1).all() and {tuple(d) for d in np.mod(cases.SHIFT_DISPLACEMENTS, 2).tolist()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
            ratios.append(ratio)
        print("scale %d, %s: ratios %s" % (scale, "BGR" if channels == 3 else "gray", ["%.3f" % x for x in ratios]))
        assert max(ratios) <= bound, ratios


def test_the_shift_scene_is_registered_exactly():
    """the camera centres displace frame n by (dx_n, dy_n) / scale source pixels: without noise a neighbour displaced by a whole source pixel
    renders the own frame's nearest samples"""
    case = cases.shift_clip(2, 1, 0, noise=0)
    src, M, m = cases.sources_and_poses(case)
    assert src == [2, 1, 3, 0, 4] and cases.SHIFT_DISPLACEMENTS[4] == (2, 3)
    r = cases.run_spec(case)
    own, far = r["planes"][0], r["planes"][4]  # frame 4 is displaced by (2, 3) fine pixels = (1, 1.5) source pixels: whole in x only
    # every fine pixel lies a quarter of a source pixel from its nearest sample on both axes (prox 4), but for the outermost ring, where the
    # position is clamped onto the border sample
    assert (own["prox"][1:-1, 1:-1] == 4).all() and (own["prox"][0, 0] == 16) and set(np.unique(far["prox"][6:-6, 6:-6]).tolist()) == {4}
    assert abs(float(np.asarray(case["truth"]).min()) - 32.0) < 1e-9 and abs(float(np.asarray(case["truth"]).max())) <= 223.0


# ---------------------------------------------------------------------------------------------------
# the library's surface
# ---------------------------------------------------------------------------------------------------
def test_the_header_names_its_definition_and_its_symbols():
    assert "tests/superres_spec_numpy.py" in HEADER_TEXT and '#include "rsdsfm_denoise.h"' in HEADER_TEXT
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER_TEXT), name
    assert "RSDSFM_SUPERRES_LAYERS_MAX 14" in HEADER_TEXT and "NOT here" in HEADER_TEXT and "CHOICES, NOT MEASUREMENTS" in HEADER_TEXT


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_symbols_are_exported_by_both_builds(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.superres_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert NEW_SYMBOLS <= set(rsdsfm.declared_symbols())
    assert not NEW_SYMBOLS & set(rsdsfm.denoise_declared_symbols())
    for name in ("superres_render_dev", "superres_render", "superres_accumulate_dev", "superres_accumulate", "superres_frame_dev", "superres_video_dev"):
        assert callable(getattr(rsdsfm.Solver, name))
    assert os.path.basename(rsdsfm.SUPERRES_HEADER_PATH) == "rsdsfm_superres.h"
    d = rsdsfm.superres_default_params()
    assert (d["scale"], d["radius"], d["strength"], d["min_overlap"], d["gain_mode"]) == (spec.SCALE_DEFAULT, spec.RADIUS_DEFAULT, spec.STRENGTH_DEFAULT,
                                                                                          spec.MIN_OVERLAP_DEFAULT, 0)
    assert ctypes.sizeof(rsdsfm.SuperresParams) == 48 and rsdsfm.SUPERRES_LAYERS_MAX == spec.LAYERS_MAX and rsdsfm.SUPERRES_RADIUS_MAX == spec.RADIUS_MAX
    assert rsdsfm.SUPERRES_SCALE_MAX == spec.SCALE_MAX and rsdsfm.SUPERRES_PROX_MAX == spec.PROX_MAX
    p = rsdsfm.SuperresParams()
    assert lib.rsdsfm_superres_params_init(ctypes.byref(p)) == 0 and p.struct_bytes == 48 and list(p.reserved) == [0] * 5


def test_launch_counts_and_host_errors(rsdsfm):
    assert rsdsfm.superres_accumulate_launches() == 1
    for r, c_, s in ((1, 64, 2), (64, 1, 2), (16385, 64, 1), (64, 16385, 1), (0, 0, 2), (64, 64, 0), (64, 64, 5), (64, 64, -1), (8193, 64, 2), (64, 5462, 3), (4097, 4097, 4)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.superres_launches(r, c_, s, 2)
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.superres_render_launches(r, c_, s)
    for r, c_, s in ((2, 2, 1), (2, 2, 4), (37, 67, 3), (720, 1280, 2), (16384, 16384, 1), (8192, 8192, 2), (5461, 5461, 3), (4096, 4096, 4)):
        one = rsdsfm.stabilize_window_launches(r, c_)
        assert rsdsfm.superres_render_launches(r, c_, s) == one
        assert rsdsfm.superres_launches(r, c_, s, 1) == one + 1
        for n in (2, 3, 5, 15):
            assert rsdsfm.superres_launches(r, c_, s, n) == n * one + 2 * (n - 1)
        for n in (0, -1, 16):
            with pytest.raises(rsdsfm.RsdsfmError):
                rsdsfm.superres_launches(r, c_, s, n)
    lib = rsdsfm.load_library()
    i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert lib.rsdsfm_superres_params_init(None) == ERR_INVALID
    # no context: refused before anything is read
    assert lib.rsdsfm_superres_render_dev(None, None, i32(3), None, None, None, f64(1), f64(1), f64(0), f64(0), i32(8), i32(8), 0, 0, i32(0), None, None, i32(2), None, None,
                                          None, None, None) == ERR_INVALID
    assert lib.rsdsfm_superres_accumulate_dev(None, None, None, None, None, None, None, i32(3), i32(8), i32(8), None, i64(0), i32(0), i32(12), None, i32(1), i32(1), None,
                                              None, None, None) == ERR_INVALID
    assert lib.rsdsfm_superres_frame_dev(None, None, i32(3), None, None, None, f64(1), f64(1), f64(0), f64(0), i32(8), i32(8), 0, 0, i32(0), i32(1), None, None, None, None,
                                         None, None, None, None) == ERR_INVALID
    assert lib.rsdsfm_superres_video_dev(None, None, i32(1), i32(8), i32(8), i32(3), f64(1), f64(1), f64(0), f64(0), None, None, None, None, None, None, None, None, 0, 0,
                                         i32(0), None, None, None, None, None, None) == ERR_INVALID


def test_evaluate_takes_the_keyword(rsdsfm):
    import inspect

    assert inspect.signature(rsdsfm.evaluate.evaluate_real_sequence).parameters["superres"].default is None
    with pytest.raises(ValueError, match="stabilize"):
        rsdsfm.evaluate.evaluate_real_sequence(None, [], superres=2)
    with pytest.raises(ValueError, match="stabilize"):
        rsdsfm.evaluate.evaluate_real_sequence(None, [], superres=(2, 1))


def test_superres_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of superres_kernels.hip, its metadata read kernel by kernel (as tests/test_denoise_cpu.py reads the denoise's): the warp kernel
    in its two instances (no LDS) and the accumulate kernel in its eight (gray / BGR, first or not, last or not; the LDS tile of 18 x 66 dwords
    and little else), a zero private segment, no VGPR and no SGPR spills"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "superres_kernels.hip")
    out = tmp_path / "superres_kernels.s"
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src,
                        "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    txt = out.read_text()
    entries = re.split(r"\n  - (?=\.)", txt[txt.index("amdhsa.kernels:"):txt.index("amdhsa.target:")])[1:]  # one YAML list item per kernel
    field = lambda e, k: re.search(r"^\s*\.%s:\s+(\S+)\s*$" % k, e, flags=re.M).group(1)
    kernels = {field(e, "name"): tuple(int(field(e, k)) for k in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"))
               for e in entries}
    names = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", open(src).read()))
    assert names == {"superres_warp_kernel", "superres_accumulate_kernel"}, sorted(names)
    warp = {n: m for n, m in kernels.items() if "superres_warp_kernel" in n}
    acc = {n: m for n, m in kernels.items() if "superres_accumulate_kernel" in n}
    assert len(warp) == 2 and len(acc) == 8 and len(kernels) == 10, sorted(kernels)
    print({n: m for n, m in kernels.items()})
    assert not {n: m for n, m in warp.items() if m != (0, 0, 0, 0)}, warp
    bad = {n: m for n, m in acc.items() if m[1:] != (0, 0, 0) or not 18 * 66 * 4 <= m[0] <= 18 * 66 * 4 + 128}
    assert not bad, bad
    assert "ds_read_b64" in txt or "ds_read2_b64" in txt  # the 3 x 6 window is read as 8-byte words
