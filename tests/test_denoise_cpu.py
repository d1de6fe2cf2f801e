"""GPU-free tests of the temporal denoise (include/rsdsfm_denoise.h): the definition (tests/denoise_spec_numpy.py) against its golden fixture,
its identities (no layer, an unrelated layer, the order of the layers), the weight's boundaries, the resolve's divide at its extremes, the
largest sums, the gain clamps, the quality on the noisy shift scene, the host functions' refusals, the exported symbols, the launch counts,
the synthetic sensor noise and the kernel's metadata."""
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

import denoise_cases as cases  # noqa: E402
import denoise_spec_numpy as spec  # noqa: E402
import stabilize_blend_spec_numpy as blend  # noqa: E402
from make_golden_denoise import digest  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_denoise_v1.npz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_denoise.h")).read()  # what this file tests is declared there: without the header, nothing here runs
NEW_SYMBOLS = {"rsdsfm_denoise_params_init", "rsdsfm_seam_overlap_sums_dev", "rsdsfm_denoise_accumulate_dev", "rsdsfm_denoise_accumulate_launches",
               "rsdsfm_denoise_frame_dev", "rsdsfm_denoise_launches", "rsdsfm_denoise_video_dev"}
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
        assert list(r["counts"]) == g[n + "counts"].tolist() and sum(r["counts"]) == r["mask"].size, n
        seen += np.array(r["counts"])
    assert (seen > 0).all()
    assert os.path.getsize(GOLDEN) <= 256 * 1024
    assert {c["frames"][0].ndim for c in all_cases} == {2, 3} and {(c["occlusion"], c["search"]) for c in all_cases} == {(0, 0), (1, 0), (1, 1)}
    assert {len(cases.sources_and_poses(c)[0]) for c in all_cases} >= {1, 2, 3, 5}
    assert not np.array_equal(g["gained/image"], g["gain-off/image"]) and np.array_equal(g["gain-off/image"], g["gain-small-overlap/image"])


def test_one_source_is_the_window_render(oracle):
    case = [c for c in cases.all_cases(oracle.pose_table) if c["name"] == "one-source"][0]
    r = cases.run_spec(case)
    ref, rmask, _ = r["ref"]
    assert np.array_equal(r["image"], ref) and np.array_equal(r["mask"], rmask) and np.array_equal(r["weight"], 16 * rmask) and r["counts"][2] == 0


@pytest.mark.parametrize("channels", [1, 3])
def test_no_layer_returns_the_reference(channels):
    ref, rmask = cases.reference(17, 65, channels)
    r = spec.denoise(ref, rmask, [])
    on = rmask != 0
    keep = on if channels == 1 else on[..., None]
    assert np.array_equal(r["image"], np.where(keep, ref, 0)) and np.array_equal(r["mask"], on.astype(np.uint8))
    assert np.array_equal(r["weight"], 16 * on) and r["counts"] == [int((~on).sum()), int(on.sum()), 0]


@pytest.mark.parametrize("channels", [1, 3])
def test_an_unrelated_layer_leaves_the_reference(channels):
    """a layer that disagrees with the own frame everywhere has w = 0: the own frame's bytes exactly, weight 16 wherever the reference is set"""
    rows, cols = 16, 64
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    rng = np.random.default_rng(4)
    ref = rng.integers(0, 100, size=shape, dtype=np.uint8)
    layer = (ref.astype(np.int64) + rng.integers(60, 150, size=shape)).astype(np.uint8)
    full = np.ones((rows, cols), dtype=np.uint8)
    r = spec.denoise(ref, full, [(layer, full), (layer[::-1].copy() | 128, full)])
    assert np.array_equal(r["image"], ref) and (r["weight"] == 16).all() and r["counts"] == [0, rows * cols, 0]


@pytest.mark.parametrize("channels", [1, 3])
def test_the_result_does_not_depend_on_the_order_of_three_layers(channels):
    ref, rmask = cases.reference(37, 67, channels)
    ls = cases.layers(ref, 37, 67, channels, 3)
    recs = [cases.records(channels)[k] for k in ("plain", "low", "small")]
    want = spec.denoise(ref, rmask, ls, recs, strength=30)
    assert min(want["counts"]) > 0
    for perm in itertools.permutations(range(3)):
        got = spec.denoise(ref, rmask, [ls[i] for i in perm], [recs[i] for i in perm], strength=30)
        for k in ("image", "mask", "weight"):
            assert np.array_equal(got[k], want[k]), perm
        assert got["counts"] == want["counts"]


def _impulse_weight(d, h, y, x, rows=5, cols=5):
    """gray, every mask set, the layer equal to the reference but for +d at the centre: D = d and N = the window's pixels in the frame, at (y, x)"""
    ref = np.full((rows, cols), 40, dtype=np.uint8)
    layer = ref.copy()
    layer[rows // 2, cols // 2] += d
    full = np.ones((rows, cols), dtype=np.uint8)
    w, _ = spec.weights(ref, full, layer, full, [blend.GAIN_ONE], h)
    return int(w[y, x])


def test_weight_boundaries():
    """w = 16 - min(16, 16 D // (h N)).  Interior of a gray frame: N = 9.  16 D one below, at and one above h N: h = 9, D = 5 (80 = 81 - 1);
    h = 16, D = 9 (144 = 144); h = 7, D = 4 (64 = 63 + 1).  D one below, at and one above h N, where w reaches 0: h = 2, D = 17, 18, 19"""
    assert _impulse_weight(5, 9, 2, 2) == 16 and _impulse_weight(9, 16, 2, 2) == 15 and _impulse_weight(4, 7, 2, 2) == 15
    assert _impulse_weight(8, 16, 2, 2) == 16 and _impulse_weight(0, 1, 2, 2) == 16
    assert _impulse_weight(17, 2, 2, 2) == 1 and _impulse_weight(18, 2, 2, 2) == 0 and _impulse_weight(19, 2, 2, 2) == 0 and _impulse_weight(215, 255, 2, 2) == 15
    # the 3 x 3 footprint: every pixel next to the impulse sees D = d, the others D = 0
    for y in range(5):
        for x in range(5):
            assert _impulse_weight(18, 2, y, x) == (0 if max(abs(y - 2), abs(x - 2)) <= 1 else 16)
    # at the frame's corner the window holds 4 pixels, at its edge 6: N follows (3 x 3 frame, the impulse in the middle)
    assert _impulse_weight(8, 2, 0, 0, 3, 3) == 16 - 16 * 8 // (2 * 4) and _impulse_weight(8, 2, 0, 1, 3, 3) == 16 - 16 * 8 // (2 * 6)
    # BGR counts three channels per pixel: D = 3 d, N = 27
    ref = np.full((5, 5, 3), 40, dtype=np.uint8)
    layer = ref.copy()
    layer[2, 2] += 9
    full = np.ones((5, 5), dtype=np.uint8)
    w, _ = spec.weights(ref, full, layer, full, [blend.GAIN_ONE] * 3, 16)
    assert int(w[2, 2]) == 15 and int(w[0, 0]) == 16  # 16 * 27 == 16 * 27
    # an invalid pixel neither counts in D nor in N, and gets no weight itself
    lmask = full.copy()
    lmask[2, 2] = 0
    w, _ = spec.weights(ref, full, layer, lmask, [blend.GAIN_ONE] * 3, 16)
    assert int(w[2, 2]) == 0 and (np.delete(w.reshape(-1), 12) == 16).all()


def test_the_resolve_divides_at_the_extremes():
    """(2 s + n) // (2 n) at n = 240: s = 61 200 is 255; 61 080 = 254.5 n rounds up to 255, one less gives 254; s = 120 is 0.5 -> 1, 119 -> 0"""
    s = np.array([61200, 61080, 61079, 120, 119, 0, 16 * 255, 16 * 200], dtype=np.uint16)
    n = np.array([240, 240, 240, 240, 240, 240, 16, 16], dtype=np.uint16)
    cells = np.stack([s, n], axis=-1).reshape(2, 4, 2)
    r = spec.resolve(cells, True)
    assert r["image"].reshape(-1).tolist() == [255, 255, 254, 1, 0, 0, 255, 200] and (r["mask"] == 1).all() and r["counts"] == [0, 2, 6]
    assert spec.resolve(np.zeros((2, 2, 4), dtype=np.uint16), False)["counts"] == [4, 0, 0]
    for nn in (16, 17, 239, 240):  # against exact rounding for every reachable sum of a stride
        ss = np.arange(0, 255 * nn + 1, 7)
        got = spec.resolve(np.stack([ss, np.full_like(ss, nn)], axis=-1).astype(np.uint16).reshape(1, -1, 2), True)["image"].reshape(-1).astype(np.int64)
        assert (2 * nn * got <= 2 * ss + nn).all() and (2 * ss + nn < 2 * nn * (got + 1)).all()


def test_radius_7_of_saturated_frames_fits_the_cells():
    ref = np.full((4, 6, 3), 255, dtype=np.uint8)
    full = np.full((4, 6), 255, dtype=np.uint8)
    r = spec.denoise(ref, full, [(ref, full)] * spec.LAYERS_MAX)
    last = r["cells"][-1]
    assert (last[..., 3] == 240).all() and (last[..., :3] == 61200).all() and last.dtype == np.uint16
    assert (r["image"] == 255).all() and (r["weight"] == 240).all() and r["counts"] == [0, 0, 24]
    assert spec.LAYERS_MAX == 2 * spec.RADIUS_MAX == 14 and 16 * (1 + spec.LAYERS_MAX) * 255 < 65536


def test_the_gain_clamps_through_the_record(rsdsfm):
    for ch in (1, 3):
        rec = cases.records(ch)
        assert spec.gains(rec["low"], ch) == [16384] * ch and spec.gains(rec["high"], ch) == [262144] * ch
        assert spec.gains(rec["small"], ch) == [65536] * ch and spec.gains(rec["plain"], ch, gain_mode=1) == [65536] * ch and spec.gains(None, ch) == [65536] * ch
        assert spec.gains(rec["zero"], ch)[0] == 65536 and spec.gains(rec["plain"], ch)[0] == 72090
        lib = rsdsfm.load_library()
        for k, r in rec.items():  # the library's host gains: the kernel's own function
            out = (ctypes.c_uint32 * 3)()
            assert lib.rsdsfm_seam_gains(r.ctypes.data_as(ctypes.c_void_p), ctypes.c_int32(ch), ctypes.c_int64(0), ctypes.c_int32(0), out) == 0
            assert list(out)[:ch] == spec.gains(r, ch), k
    # a gained layer: k = min(255, (G L + 32768) >> 16)
    k = spec.gained(np.array([[0, 1, 100, 255]], dtype=np.uint8), [262144])
    assert k.reshape(-1).tolist() == [0, 4, 255, 255]
    assert spec.gained(np.array([[3, 255]], dtype=np.uint8), [16384]).reshape(-1).tolist() == [1, 64]


# ---------------------------------------------------------------------------------------------------
# quality
# ---------------------------------------------------------------------------------------------------
def _ratio(case):
    r = cases.run_spec(case)
    q = case["q"]
    cols_ok = cases.shift_seen_by_all(case)
    clean = case["clean"][q].astype(np.int64)
    assert (r["mask"] == 1).all() and np.array_equal(r["ref"][0], case["frames"][q])  # the own render is the own frame: the renders align exactly
    err = lambda img: np.abs(img.astype(np.int64) - clean)[:, cols_ok].mean()
    return err(r["image"]) / err(case["frames"][q])


@pytest.mark.parametrize("channels", [3, 1])
def test_the_noisy_shift_scene_is_denoised(channels):
    """five frames of the shift scene, texture bytes 32 .. 223, i.i.d. integer noise in [-6, 6]; over the columns all five frames see the mean
    absolute error against the clean texture is at most 0.55 of the noisy own frame's at K = 2, h = 12.  (The weight rule on aligned copies
    gives 0.42 - 0.44.)  K = 7 needs fifteen frames to differ from K = 2: the same scene with fifteen frames of 128 columns, frame 7, where all
    fifteen see 16 columns (0.23 - 0.24 on aligned copies); asserted only to be smaller than K = 2 on the same frame"""
    ratios = [_ratio(cases.shift_clip(seed, channels)) for seed in range(5)]
    print("K = 2, h = 12, %s: ratios %s" % ("BGR" if channels == 3 else "gray", ["%.3f" % x for x in ratios]))
    assert max(ratios) <= 0.55, ratios
    wide = dict(nframes=15, cols=128, q=7)
    k7 = _ratio(cases.shift_clip(0, channels, radius=7, **wide))
    two = cases.shift_clip(0, channels, radius=2, **wide)
    r = cases.run_spec(two)
    cols_ok = cases.shift_seen_by_all(cases.shift_clip(0, channels, radius=7, **wide))  # the K = 7 columns, for both
    clean = two["clean"][7].astype(np.int64)
    err = lambda img: np.abs(img.astype(np.int64) - clean)[:, cols_ok].mean()
    k2 = err(r["image"]) / err(two["frames"][7])
    print("fifteen frames, frame 7: K = 2 %.3f, K = 7 %.3f over %d columns" % (k2, k7, int(cols_ok.sum())))
    assert int(cols_ok.sum()) == 16 and k7 < k2


# ---------------------------------------------------------------------------------------------------
# the library's surface
# ---------------------------------------------------------------------------------------------------
def test_the_header_names_its_definition_and_its_symbols():
    assert "tests/denoise_spec_numpy.py" in HEADER_TEXT and '#include "rsdsfm_shutter.h"' in HEADER_TEXT
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER_TEXT), name
    assert "d_counts3_or_null" in HEADER_TEXT and "RSDSFM_DENOISE_LAYERS_MAX 14" in HEADER_TEXT and "NOT here" in HEADER_TEXT


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_symbols_are_exported_by_both_builds(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.denoise_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    assert NEW_SYMBOLS <= set(rsdsfm.declared_symbols())
    assert not NEW_SYMBOLS & set(rsdsfm.shutter_declared_symbols())
    for name in ("seam_overlap_sums_dev", "denoise_accumulate_dev", "denoise_accumulate", "denoise_frame_dev", "denoise_video_dev"):
        assert callable(getattr(rsdsfm.Solver, name))
    assert os.path.basename(rsdsfm.DENOISE_HEADER_PATH) == "rsdsfm_denoise.h"
    d = rsdsfm.denoise_default_params()
    assert (d["radius"], d["strength"], d["min_overlap"], d["gain_mode"], d["occlusion"]) == (spec.RADIUS_DEFAULT, spec.STRENGTH_DEFAULT, spec.MIN_OVERLAP_DEFAULT, 0, 0)
    assert ctypes.sizeof(rsdsfm.DenoiseParams) == 48 and rsdsfm.DENOISE_LAYERS_MAX == spec.LAYERS_MAX and rsdsfm.DENOISE_RADIUS_MAX == spec.RADIUS_MAX
    p = rsdsfm.DenoiseParams()
    assert lib.rsdsfm_denoise_params_init(ctypes.byref(p)) == 0 and p.struct_bytes == 48 and list(p.reserved) == [0, 0, 0, 0]


def test_launch_counts_and_host_errors(rsdsfm):
    assert rsdsfm.denoise_accumulate_launches() == 1
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385), (0, 0)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.denoise_launches(r, c_, 2)
    for r, c_ in ((2, 2), (37, 67), (720, 1280), (16384, 16384)):
        one = rsdsfm.stabilize_window_launches(r, c_)
        assert rsdsfm.denoise_launches(r, c_, 1) == one + 1
        for n in (2, 3, 5, 15):
            assert rsdsfm.denoise_launches(r, c_, n) == n * one + 2 * (n - 1)
        for n in (0, -1, 16):
            with pytest.raises(rsdsfm.RsdsfmError):
                rsdsfm.denoise_launches(r, c_, n)
    lib = rsdsfm.load_library()
    i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert lib.rsdsfm_denoise_params_init(None) == ERR_INVALID
    # no context: refused before anything is read
    assert lib.rsdsfm_seam_overlap_sums_dev(None, None, None, None, None, i32(3), i32(8), i32(8), None) == ERR_INVALID
    assert lib.rsdsfm_denoise_accumulate_dev(None, None, None, None, None, i32(3), i32(8), i32(8), None, i64(0), i32(0), i32(12), None, i32(1), i32(1), None, None, None,
                                             None) == ERR_INVALID
    assert lib.rsdsfm_denoise_frame_dev(None, None, i32(3), None, None, None, f64(1), f64(1), f64(0), f64(0), i32(8), i32(8), 0, 0, i32(0), i32(1), None, None, None, None,
                                        None, None, None, None) == ERR_INVALID
    assert lib.rsdsfm_denoise_video_dev(None, None, i32(1), i32(8), i32(8), i32(3), f64(1), f64(1), f64(0), f64(0), None, None, None, None, None, None, None, None, 0, 0,
                                        i32(0), None, None, None, None, None, None) == ERR_INVALID


def test_evaluate_takes_the_keyword(rsdsfm):
    import inspect

    assert inspect.signature(rsdsfm.evaluate.evaluate_real_sequence).parameters["denoise"].default is None
    with pytest.raises(ValueError, match="stabilize"):
        rsdsfm.evaluate.evaluate_real_sequence(None, [], denoise=2)
    with pytest.raises(ValueError, match="stabilize"):
        rsdsfm.evaluate.evaluate_real_sequence(None, [], denoise=(2, 12))


def test_synthetic_sensor_noise_is_seeded_and_off_by_default(rsdsfm):
    synth = rsdsfm.synth
    v, w, k = synth.default_motion()
    K = (60.0, 60.0, 24.0, 16.0)
    plain, flow, mask = synth.render_sequence(3, 32, 48, K, v, w, k)
    off, flow0, mask0 = synth.render_sequence(3, 32, 48, K, v, w, k, noise=None, noise_seed=99)
    assert np.array_equal(off, plain) and np.array_equal(flow0, flow) and np.array_equal(mask0, mask)
    assert np.array_equal(synth.render_sequence(3, 32, 48, K, v, w, k, noise=0)[0], plain)
    a = synth.render_sequence(3, 32, 48, K, v, w, k, noise=6, noise_seed=1)[0]
    b = synth.render_sequence(3, 32, 48, K, v, w, k, noise=6, noise_seed=1)[0]
    c = synth.render_sequence(3, 32, 48, K, v, w, k, noise=6, noise_seed=2)[0]
    assert np.array_equal(a, b) and not np.array_equal(a, c) and a.dtype == np.uint8 and a.shape == plain.shape
    d = a.astype(np.int64) - plain
    inner = (plain >= 6) & (plain <= 249)
    assert np.abs(d).max() == 6 and set(np.unique(d[inner]).tolist()) == set(range(-6, 7))
    assert np.array_equal(synth.render_sequence(2, 32, 48, K, v, w, k, noise=6, noise_seed=1)[0], a[:2])  # a frame's noise does not depend on the frames behind it
    g = synth.render_sequence(3, 32, 48, K, v, w, k, gains=[1.0, 1.2, 0.8], noise=3)[0]  # after the exposure gain
    assert np.abs(g.astype(np.int64) - synth.render_sequence(3, 32, 48, K, v, w, k, gains=[1.0, 1.2, 0.8])[0]).max() <= 3
    with pytest.raises(ValueError):
        synth.render_sequence(3, 32, 48, K, v, w, k, noise=-1)


def test_denoise_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of denoise_kernels.hip, its metadata read kernel by kernel (as tests/test_shutter_cpu.py reads the shutter's): the one kernel in
    its eight instances (gray / BGR, first or not, last or not), a zero private segment, no VGPR and no SGPR spills, the LDS tile of 18 x 66
    dwords and little else"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "denoise_kernels.hip")
    out = tmp_path / "denoise_kernels.s"
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src,
                        "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    txt = out.read_text()
    entries = re.split(r"\n  - (?=\.)", txt[txt.index("amdhsa.kernels:"):txt.index("amdhsa.target:")])[1:]  # one YAML list item per kernel
    field = lambda e, k: re.search(r"^\s*\.%s:\s+(\S+)\s*$" % k, e, flags=re.M).group(1)
    kernels = {field(e, "name"): tuple(int(field(e, k)) for k in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"))
               for e in entries}
    names = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", open(src).read()))
    assert names == {"denoise_accumulate_kernel"} and len(kernels) == 8, (sorted(kernels), sorted(names))
    assert all("denoise_accumulate_kernel" in n for n in kernels)
    print({n: m for n, m in kernels.items()})
    bad = {n: m for n, m in kernels.items() if m[1:] != (0, 0, 0) or not 18 * 66 * 4 <= m[0] <= 18 * 66 * 4 + 128}
    assert not bad, bad
    assert "ds_read_b64" in txt or "ds_read2_b64" in txt  # the 3 x 6 window is read as 8-byte words
