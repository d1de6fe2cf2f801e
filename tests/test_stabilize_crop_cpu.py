"""CPU: the crop's definition (tests/stabilize_crop_spec_numpy.py) -- the window against a brute-force search and its monotonicity on random
masks, the windows known exactly, the exact zoom-2 case on the stabiliser's shift case, the full-frame window against the stabiliser and
the fill bit for bit, its accuracy against an analytic truth, the golden fixture -- and the ABI (include/rsdsfm_stabilize_crop.h): exported by
both library builds, the argument errors that need no GPU, every kernel without a private segment or spills."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rectify_dense_spec_numpy as dense
import stabilize_crop_cases as cases
import stabilize_crop_spec_numpy as spec
import stabilize_fill_spec_numpy as fill
import stabilize_spec_numpy as stab
from conftest import ROOT

NEW_SYMBOLS = {"rsdsfm_stabilize_crop_params_init", "rsdsfm_crop_window_dev", "rsdsfm_crop_window_launches", "rsdsfm_stabilize_window_frame_dev",
               "rsdsfm_stabilize_window_launches", "rsdsfm_stabilize_video_cropped_dev"}
KERNELS = {"crop_rowscan_kernel", "crop_colscan_kernel", "crop_search_kernel", "stabilize_window_warp_kernel", "stabilize_window_warp_gray_kernel"}
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_stabilize_crop_v1.npz")
ERR_INVALID = -1  # RSDSFM_ERR_INVALID (include/rsdsfm.h)


def _brute_fits(common, r, c, h, max_empty, margin):
    rows, cols = common.shape
    w = (h * cols) // rows
    if w < 1 or r + h > rows or c + w > cols:
        return False
    box = common[max(r - margin, 0):min(r + h + margin, rows), max(c - margin, 0):min(c + w + margin, cols)]
    return int((~box).sum()) <= max_empty


def _brute_window(masks, max_empty, margin):
    """every anchor, every height, the issue's order of preference written as a sort key"""
    common = np.all(np.asarray(masks) != 0, axis=0)
    rows, cols = common.shape
    best = None
    for r in range(rows):
        for c in range(cols):
            for h in range(1, rows + 1):
                if _brute_fits(common, r, c, h, max_empty, margin):
                    w = (h * cols) // rows
                    k = (-h, abs(2 * r + h - rows) + abs(2 * c + w - cols), r, c)
                    if best is None or k < best[0]:
                        best = (k, (r, c, h, w))
    return best[1] if best else (0, 0, 0, 0)


# ---------------------------------------------------------------------------------------------------
# the window
# ---------------------------------------------------------------------------------------------------
def test_window_against_brute_force_and_monotone():
    """20 random masks up to 30 x 30, 1 .. 3 planes, margins 0 .. 3, max_empty 0 .. 2: the vectorised binary search gives the brute-force
    search's window, and for every anchor fitting is monotone in the height (what the binary search rests on)"""
    rng = np.random.default_rng(77)
    found = 0
    for i in range(20):
        rows, cols = int(rng.integers(2, 31)), int(rng.integers(2, 31))
        planes, margin, max_empty = int(rng.integers(1, 4)), int(rng.integers(0, 4)), int(rng.integers(0, 3))
        masks = cases.random_masks(rows, cols, planes, float(rng.choice([0.0, 0.01, 0.03, 0.1])), 1000 + i, set_value=int(rng.choice([1, 255])))
        got = spec.crop_window(masks, max_empty, margin)
        assert got == _brute_window(masks, max_empty, margin), (i, rows, cols, margin, max_empty)
        found += got[2] > 0
        common = spec.common_mask(masks)
        H = spec.largest_heights(spec.empties_table(common), max_empty, margin)
        for r in range(rows):
            for c in range(cols):
                f = [_brute_fits(common, r, c, h, max_empty, margin) for h in range(1, rows + 1) if (h * cols) // rows >= 1]
                assert f == sorted(f, reverse=True), (i, r, c)  # True ... True False ... False
                assert int(H[r, c]) == (sum(f) + (rows + cols - 1) // cols - 1 if any(f) else 0), (i, r, c)
    assert found >= 15


@pytest.mark.parametrize("case", cases.exact_windows(), ids=lambda c: c[0])
def test_exact_windows(case):
    _, masks, max_empty, margin, want = case
    assert spec.crop_window(masks, max_empty, margin) == want
    assert spec.crop_window(np.concatenate([masks, np.full_like(masks, 255)]), max_empty, margin) == want  # a plane that is set everywhere changes nothing


def test_key_orders_the_windows():
    rows, cols = 16384, 16384
    k = spec.window_key(0, 0, 16384, rows, cols)
    assert k < 1 << 60 and spec.decode_key(k, rows, cols) == (0, 0, 16384, 16384) and spec.decode_key(0, 7, 5) == (0, 0, 0, 0)
    rows, cols = 6, 9
    ks = [spec.window_key(r, c, 3, rows, cols) for r, c in ((1, 0), (1, 5), (2, 0), (2, 5), (0, 0))]
    assert ks == sorted(ks, reverse=True) and spec.window_key(5, 8, 4, rows, cols) > ks[0]  # the height first
    assert spec.decode_key(ks[0], rows, cols) == (1, 0, 3, 4)


# ---------------------------------------------------------------------------------------------------
# one frame through a window
# ---------------------------------------------------------------------------------------------------
def test_exact_zoom_two_on_the_shift_case():
    """D is exactly (8, -4); through (4, 14, 12, 20) the positions are exactly 6 + ix / 2 - 0.25 and 8 + iy / 2 - 0.25, inside the frame
    everywhere, after 1 iteration and after 16: the zoom does not touch the contraction"""
    z = cases.zoom2_case()
    for it in (1, 3, 16):
        r = spec.stabilize_frame_window(z["image"], z["depth"], z["R"], z["t"], z["K"], z["M"], z["m"], z["window"], iterations=it)
        assert np.array_equal(r["disp"], np.broadcast_to(np.array([8.0, -4.0], dtype=np.float32), r["disp"].shape))
        px, py = spec.inverse_positions_window(r["disp"], it, z["window"])
        assert np.array_equal(px, z["px"]) and np.array_equal(py, z["py"])
        assert r["mask"].all() and r["valid"] == 24 * 40
        assert np.array_equal(r["image"], dense.saturate_u8(dense.bilinear(z["image"], z["px"], z["py"])))
    assert (r["image"][0::2, 0::2] != r["image"][1::2, 1::2]).any()


def test_full_frame_window_is_the_unwindowed_call(oracle):
    rows, cols = 33, 70
    cc = cases.clip_case(oracle.pose_table, rows, cols)
    full = (0, 0, rows, cols)
    tx, ty = spec.window_targets(full, rows, cols)
    iy, ix = np.mgrid[0:rows, 0:cols].astype(np.float64)
    assert np.array_equal(tx, ix) and np.array_equal(ty, iy)
    a = stab.stabilize_frame(cc["images"][1], cc["depths"][1], cc["Rs"][1], cc["ts"][1], cc["K"], cc["M"][1], cc["m"][1])
    b = spec.stabilize_frame_window(cc["images"][1], cc["depths"][1], cc["Rs"][1], cc["ts"][1], cc["K"], cc["M"][1], cc["m"][1], full)
    assert np.array_equal(a["image"], b["image"]) and np.array_equal(a["mask"], b["mask"]) and 0 < a["valid"] == b["valid"] < rows * cols
    px, py = spec.inverse_positions_window(b["disp"], 3, full)
    qx, qy = dense.inverse_positions(a["disp"], 3)
    assert np.array_equal(px, qx, equal_nan=True) and np.array_equal(py, qy, equal_nan=True)
    M, m = fill.neighbour_pose(cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], 1, 2)
    outs = []
    for fn, extra in ((fill.fill_from, ()), (spec.fill_from_window, (full,))):
        out, mask, source = a["image"].copy(), a["mask"].copy(), a["mask"].copy()
        n = fn(out, mask, source, cc["images"][2], cc["depths"][2], cc["Rs"][2], cc["ts"][2], cc["K"], M, m, 3, *extra)
        outs.append((out, mask, source, n))
    assert outs[0][3] == outs[1][3] > 0 and all(np.array_equal(x, y) for x, y in zip(outs[0][:3], outs[1][:3]))
    # the whole frame: zeroed planes + the own frame with id 1 + the neighbours = stabilize_filled_frame
    want = fill.stabilize_filled_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], 1, cc["M"][1],
                                       cc["m"][1])
    got = spec.stabilize_cropped_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], 1, cc["M"][1],
                                       cc["m"][1], full)
    assert got["counts"] == want["counts"] and all(np.array_equal(got[k], want[k]) for k in ("image", "mask", "source"))


def test_no_window_and_no_depth_offer_nothing(oracle):
    rows, cols = 33, 70
    cc = cases.clip_case(oracle.pose_table, rows, cols)
    r = spec.stabilize_cropped_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], 1, cc["M"][1],
                                     cc["m"][1], (0, 0, 0, 0))
    assert r["counts"] == [rows * cols, 0, 0, 0, 0, 0] and not r["image"].any() and not r["mask"].any() and not r["source"].any()
    _, _, none_valid = cases.inputs(rows, cols, none_valid=True)
    out, mask, source = (np.full(s, 9, dtype=np.uint8) for s in ((rows, cols, 3), (rows, cols), (rows, cols)))
    mask[:] = 0
    assert spec.fill_from_window(out, mask, source, cc["images"][2], none_valid, cc["Rs"][2], cc["ts"][2], cc["K"], cc["M"][2], cc["m"][2], 1, (3, 5, 20, 42)) == 0
    assert (out == 9).all() and not mask.any() and (source == 9).all()
    for bad in ((0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 5, 5), (30, 0, 4, 4), (0, 60, 4, 11)):
        with pytest.raises(AssertionError):
            spec.window_targets(bad, rows, cols)


# ---------------------------------------------------------------------------------------------------
# golden fixture, accuracy
# ---------------------------------------------------------------------------------------------------
def test_golden_fixture_is_the_spec(oracle):
    """tests/golden/make_golden_stabilize_crop.py wrote the spec's outputs; recomputed here from the cases' own inputs, so an edit of the
    spec cannot pass unnoticed"""
    assert os.path.getsize(GOLDEN) < 200 * 1024
    g = np.load(GOLDEN)
    names = sorted(set(k.split("/")[0] for k in g.files))
    assert names == ["24x40", "33x70", "5x3", "mask33x70", "mask7x5", "mask96x128"]
    for n in names:
        get = lambda k: g[n + "/" + k]
        if n.startswith("mask"):
            rows, cols = (int(x) for x in n[4:].split("x"))
            planes, seed, max_empty, margin = (int(x) for x in get("params"))
            m = cases.random_masks(rows, cols, planes, float(get("empty")), seed)
            assert np.array_equal(np.packbits(m != 0), get("masks"))
            assert spec.crop_window(m, max_empty, margin) == tuple(get("window").tolist())
            continue
        rows, cols = (int(x) for x in n.split("x"))
        ch, q, radius, mode, q5, it, margin = (int(x) for x in get("modes"))
        cc = cases.clip_case(oracle.pose_table, rows, cols, channels=ch)
        masks = np.unpackbits(get("masks"))[:4 * rows * cols].reshape(4, rows, cols)
        for p in range(4):
            if radius:
                r = fill.stabilize_filled_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], p,
                                                cc["M"][p], cc["m"][p], radius=radius, mode=mode, q5_mode=q5, iterations=it)
            else:
                r = stab.stabilize_frame(cc["images"][p], cc["depths"][p], cc["Rs"][p], cc["ts"][p], cc["K"], cc["M"][p], cc["m"][p], mode=mode, q5_mode=q5,
                                         iterations=it)
            assert np.array_equal(r["mask"], masks[p]), (n, p)
        window = spec.crop_window(masks, 0, margin)
        assert window == tuple(get("window").tolist()) and window[2] > 0
        r = spec.stabilize_cropped_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], q, cc["M"][q],
                                         cc["m"][q], window, radius=radius, mode=mode, q5_mode=q5, iterations=it)
        for k in ("image", "mask", "source"):
            assert np.array_equal(r[k], get("out_" + k)), (n, k)
        assert r["counts"] == get("out_counts").tolist() and sum(r["counts"]) == rows * cols and len(r["counts"]) == 2 + 2 * radius
    assert g["33x70/out_counts"][2:].sum() > 0  # a neighbour was needed inside the window


def test_accuracy_against_the_analytic_truth(oracle, rsdsfm):
    """stabilize_fill_cases.static_scene (two frames of one static scene from two known poses; the own frame's virtual camera is turned by
    0.05 rad) through the window the search finds on the FILLED frame's mask.  Truth, independent of stages A and C: the neighbour's forward
    map on the TRUE depth in float64, inverted by 50 fixed-point iterations with synth._bilinear AT THE WINDOW'S TARGETS, and the texture
    evaluated analytically there.  Over the pixels the neighbour offers through the window (it is rendered alone, onto a zeroed mask): the
    position error after 3 iterations and the mean absolute error below the values measured here on the CPU plus half of them
    (stabilize_crop_cases.ACC_*); and over the cropped frame (the window leaves out the corner nobody saw and the band the neighbour filled, so
    every pixel is the own frame's) the mean absolute error against the same truth below that bound too -- both frames show one scene.
    Measured: window (0, 0, 90, 120); the neighbour alone 12288 pixels, position error 0.265833 px (bound 0.398750), mean abs error 0.359596
    (bound 0.539394); the cropped frame's counts [0, 12288, 0, 0], its mean abs error 0.3521."""
    sc0 = cases.static_scene(rsdsfm.synth, oracle.pose_table)
    filled = fill.stabilize_filled_frame(sc0["images"], sc0["depths"], sc0["Rs"], sc0["ts"], sc0["K"], sc0["A"], sc0["c"], sc0["As"], sc0["cs"], sc0["scales"], 0,
                                         sc0["M"], sc0["m"], radius=1, iterations=3)
    window = spec.crop_window(filled["mask"][None])
    rows, cols = filled["mask"].shape
    assert window[2] >= 0.8 * rows and window[2] < rows  # a real crop, and not much of one
    sc = cases.static_scene_window(rsdsfm.synth, oracle.pose_table, window)
    cand = spec.stabilize_frame_window(sc["images"][1], sc["depths"][1], sc["Rs"][1], sc["ts"][1], sc["K"], sc["Mn"], sc["mn"], window, iterations=3)
    qx, qy = spec.inverse_positions_window(cand["disp"], 3, window)
    ok = cand["mask"] == 1
    pos = np.sqrt((qx - sc["px_w"]) ** 2 + (qy - sc["py_w"]) ** 2)[ok].max()
    mae = np.abs(cand["image"].astype(np.float64) - sc["truth_w"])[ok].mean()
    r = spec.stabilize_cropped_frame(sc["images"], sc["depths"], sc["Rs"], sc["ts"], sc["K"], sc["A"], sc["c"], sc["As"], sc["cs"], sc["scales"], 0, sc["M"], sc["m"],
                                     window, radius=1, iterations=3)
    err = np.abs(r["image"].astype(np.float64) - sc["truth_w"])
    taken = r["mask"] == 1
    print("window %s; neighbour alone: %d pixels, position error %.6f px (bound %.6f), mean abs error %.6f (bound %.6f); cropped frame counts %s, mean abs "
          "error %.4f" % (window, int(ok.sum()), pos, cases.ACC_BOUND, mae, cases.ACC_MAE_BOUND, r["counts"], err[taken].mean()))
    assert ok.sum() > 0.9 * ok.size and pos < cases.ACC_BOUND and mae < cases.ACC_MAE_BOUND
    assert r["counts"][0] <= 8 and sum(r["counts"]) == taken.size and filled["counts"][0] > 100  # the un-cropped frame has pixels nobody saw
    assert err[taken].mean() < cases.ACC_MAE_BOUND


# ---------------------------------------------------------------------------------------------------
# ABI and kernel metadata
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_stabilize_crop_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.stabilize_crop_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    for other in (rsdsfm.declared_symbols(), rsdsfm.video_declared_symbols(), rsdsfm.rectify_video_declared_symbols(), rsdsfm.flow_declared_symbols(),
                  rsdsfm.rectify_dense_declared_symbols(), rsdsfm.flow_check_declared_symbols(), rsdsfm.trajectory_declared_symbols(),
                  rsdsfm.fuse_declared_symbols(), rsdsfm.stabilize_declared_symbols(), rsdsfm.stabilize_fill_declared_symbols()):
        assert not NEW_SYMBOLS & set(other)
    assert rsdsfm.stabilize_crop_default_params() == dict(max_empty=0, margin=spec.MARGIN_DEFAULT) == dict(max_empty=0, margin=1)
    assert ctypes.sizeof(rsdsfm.StabilizeCropParams) == 32
    p = rsdsfm.StabilizeCropParams()
    assert lib.rsdsfm_stabilize_crop_params_init(None) != rsdsfm.OK
    assert lib.rsdsfm_stabilize_crop_params_init(ctypes.byref(p)) == rsdsfm.OK
    assert (p.max_empty, p.margin, p.struct_bytes, list(p.reserved)) == (0, 1, 32, [0, 0, 0, 0])
    assert os.path.exists(rsdsfm.STABILIZE_CROP_HEADER_PATH)
    for name in ("crop_window", "crop_window_dev", "stabilize_window_frame_dev", "stabilize_cropped", "stabilize_video_cropped_dev"):
        assert callable(getattr(rsdsfm.Solver, name))


def test_host_argument_errors_and_launch_counts(rsdsfm):
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385), (0, 0)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.crop_window_launches(r, c_)
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.stabilize_window_launches(r, c_)
    for r, c_ in ((2, 2), (300, 400), (720, 1280), (16384, 16384)):
        assert rsdsfm.crop_window_launches(r, c_) == 3
        assert rsdsfm.stabilize_window_launches(r, c_) == rsdsfm.stabilize_fill_launches(r, c_) == rsdsfm.rectify_dense_launches(r, c_)
    lib = rsdsfm.load_library()
    w = (ctypes.c_int32 * 4)(7, 7, 7, 7)
    planes = (ctypes.c_void_p * 1)(None)
    assert lib.rsdsfm_crop_window_dev(None, planes, ctypes.c_int32(1), ctypes.c_int32(8), ctypes.c_int32(8), None, w) == ERR_INVALID  # no context
    assert list(w) == [7, 7, 7, 7]
    assert lib.rsdsfm_stabilize_window_frame_dev(*([None] * 6), *[ctypes.c_double(1.0)] * 4, *[ctypes.c_int32(8)] * 2, 0, 0, ctypes.c_int32(0), None, None,
                                                 ctypes.c_int32(1), w, None, None, None, None) == ERR_INVALID


def test_stabilize_crop_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of stabilize_crop_kernels.hip, its metadata read kernel by kernel (as tests/test_stabilize_fill_cpu.py reads the fill's):
    exactly the five kernels, a zero private segment, no VGPR and no SGPR spills, LDS at most 64 KB"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "stabilize_crop_kernels.hip")
    out = tmp_path / "stabilize_crop_kernels.s"
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src,
                        "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    txt = out.read_text()
    entries = re.split(r"\n  - (?=\.)", txt[txt.index("amdhsa.kernels:"):txt.index("amdhsa.target:")])[1:]  # one YAML list item per kernel
    field = lambda e, k: re.search(r"^\s*\.%s:\s+(\S+)\s*$" % k, e, flags=re.M).group(1)
    kernels = {field(e, "name"): tuple(int(field(e, k)) for k in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"))
               for e in entries}
    names = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", open(src).read()))
    assert names == KERNELS and len(kernels) == len(KERNELS), (sorted(kernels), sorted(names))
    for k in KERNELS:
        assert any(k in n for n in kernels), k
    bad = {n: m for n, m in kernels.items() if m[1:] != (0, 0, 0) or m[0] > 65536}
    assert not bad, bad
    print({n: (m, field(e, "vgpr_count"), field(e, "sgpr_count")) for (n, m), e in zip(kernels.items(), entries)})
