"""CPU: the border fill's definition (tests/stabilize_fill_spec_numpy.py) -- the two exact cases on the stabiliser's shift case, the order of the
candidates at the clip's ends, the neighbour's pose against the chain, precedence, the candidates that offer nothing, its accuracy against an
analytic truth, the golden fixture -- the library's host function against it, and the ABI (include/rsdsfm_stabilize_fill.h): exported by
both library builds, every kernel without a private segment or spills."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rectify_dense_spec_numpy as dense
import stabilize_fill_cases as cases
import stabilize_fill_spec_numpy as spec
import stabilize_spec_numpy as stab
from conftest import ROOT

NEW_SYMBOLS = {"rsdsfm_stabilize_fill_params_init", "rsdsfm_neighbour_poses", "rsdsfm_stabilize_fill_frame_dev", "rsdsfm_stabilize_fill_launches",
               "rsdsfm_stabilize_video_filled_dev"}
KERNELS = {"stabilize_fill_warp_kernel", "stabilize_fill_warp_gray_kernel"}
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_stabilize_fill_v1.npz")
ERR_INVALID = -1  # RSDSFM_ERR_INVALID (include/rsdsfm.h)


def _own(s):
    own = stab.stabilize_frame(s["image"], s["depth"], s["R"], s["t"], s["K"], s["M"], s["m"])
    return own["image"].copy(), own["mask"].copy(), own["mask"].copy()


# ---------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full", "partial"])
def test_exact_cases_on_the_shift_case(name):
    """full: the neighbour as it is fills exactly the 320 pixels the own frame leaves, with its own bytes: counts (0, 640, 320).  partial: seen
    with m = (-1, 0.5, 0) it fills columns 0 .. 7 of rows 4 .. 19 and columns 0 .. 31 of rows 20 .. 23 and leaves 64: counts (64, 640, 256)"""
    s = cases.shift_fill_case()
    e = s[name]
    out, mask, source = _own(s)
    assert int(mask.sum()) == 640
    n = spec.fill_from(out, mask, source, s["neighbour"], s["depth"], s["R"], s["t"], s["K"], e["M"], e["m"], 2)
    assert (mask.size - 640 - n, 640, n) == e["counts"]
    assert np.array_equal(out, e["want"]) and np.array_equal(mask == 1, (s["mask"] == 1) | e["take"])
    assert np.array_equal(source, s["mask"] + 2 * e["take"].astype(np.uint8))
    if name == "full":
        assert np.array_equal(out[e["take"]], s["neighbour"][e["take"]]) and mask.all()
    else:
        rows = np.nonzero(e["take"].any(axis=1))[0]
        assert rows.min() == 4 and rows.max() == 23 and e["take"][4:20, :8].all() and e["take"][20:, :32].all() and int(e["take"].sum()) == 256
    # the whole frame through stabilize_filled_frame: a clip of two pairs whose frame 1 is the neighbour, with poses that give exactly (M, m)
    A, c = np.stack([np.eye(3)] * 3), np.stack([np.zeros(3), e["m"] - s["m"], np.zeros(3)])  # c~_0 = c_0 - own m, c_1 - c~_0 = e.m
    As, cs = A.copy(), np.stack([-s["m"], c[1], np.zeros(3)])
    r = spec.stabilize_filled_frame([s["image"], s["neighbour"]], [s["depth"]] * 2, [s["R"]] * 2, [s["t"]] * 2, s["K"], A, c, As, cs, np.ones(2), 0, s["M"], s["m"],
                                    radius=1)
    assert r["counts"] == [e["counts"][0], 640, 0, e["counts"][2]]  # frame 1 is the NEXT frame: source id 3
    assert np.array_equal(r["image"], e["want"]) and np.array_equal(r["source"], s["mask"] + 3 * e["take"].astype(np.uint8))


def test_neighbour_order_at_the_clips_ends():
    assert spec.neighbour_order(2, 6, 2) == [1, 3, 0, 4]
    assert spec.neighbour_order(0, 6, 2) == [1, 2]  # no previous frame
    assert spec.neighbour_order(5, 6, 2) == [4, 3]  # frame 6, the clip's last, has no pair: never listed
    assert spec.neighbour_order(4, 6, 3) == [3, 5, 2, 1]
    assert spec.neighbour_order(0, 1, 16) == []
    assert [spec.source_id(j) for j in (-1, 1, -2, 2, -16, 16)] == [2, 3, 4, 5, 32, 33]
    for q in range(6):
        order = spec.neighbour_order(q, 6, 3)
        assert q not in order and 6 not in order and len(set(order)) == len(order)
        assert [abs(n - q) for n in order] == sorted(abs(n - q) for n in order)  # nearer first


def test_neighbour_pose_on_the_golden_path():
    """the same world point through frame n and through the virtual camera of frame q: A~_q (M X + m) S_n + c~_q = A_n X S_n + c_n.  The golden
    path has a broken link, which carries its scale over, as in the chain"""
    p = cases.golden_path()
    A, c, S = p["A"], p["c"], p["scales"]
    assert S[5] == S[4]  # the broken link
    rng = np.random.default_rng(9)
    for translation in (True, False):
        As, cs = stab.smooth_path(A, c, p["sigma"], translation=translation)
        assert translation or np.array_equal(cs, c)
        for q in range(len(S)):
            for n in spec.neighbour_order(q, len(S), 3):
                M, m = spec.neighbour_pose(A, c, As, cs, S, q, n)
                X = rng.normal(size=3) * 2.0
                assert np.allclose(As[q] @ (M @ X + m) * S[n] + cs[q], A[n] @ X * S[n] + c[n], rtol=0, atol=1e-12)
                assert np.abs(m).max() > 0  # the baseline is real also when the translation is not smoothed
    with pytest.raises(AssertionError):
        spec.neighbour_pose(A, c, As, cs, np.where(np.arange(len(S)) == 2, np.nan, S), 1, 2)


def test_precedence_the_earlier_neighbour_wins(oracle):
    cc = cases.clip_case(oracle.pose_table, 33, 70)
    q = 2
    order = spec.neighbour_order(q, 4, 2)
    assert order == [1, 3, 0]
    r = spec.stabilize_filled_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], q, cc["M"][q],
                                    cc["m"][q])
    own = r["own"]
    cands = {}
    for n in order:
        M, m = spec.neighbour_pose(cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], q, n)
        cands[n] = stab.stabilize_frame(cc["images"][n], cc["depths"][n], cc["Rs"][n], cc["ts"][n], cc["K"], M, m)
    empty = own["mask"] == 0
    both = empty & (cands[1]["mask"] == 1) & (cands[3]["mask"] == 1)
    assert both.sum() > 0 and (cands[1]["image"][both] != cands[3]["image"][both]).any()  # two offers that differ
    assert (r["source"][both] == 2).all() and np.array_equal(r["image"][both], cands[1]["image"][both])
    only3 = empty & (cands[1]["mask"] == 0) & (cands[3]["mask"] == 1)
    assert only3.sum() > 0 and (r["source"][only3] == 3).all() and np.array_equal(r["image"][only3], cands[3]["image"][only3])
    assert np.array_equal(r["image"][~empty], own["image"][~empty]) and (r["source"][~empty] == 1).all()
    assert np.array_equal(r["source"] != 0, r["mask"] == 1) and sum(r["counts"]) == 33 * 70
    assert [int((r["source"] == i).sum()) for i in range(6)] == r["counts"] and r["counts"][5] == 0  # offset +2 is the clip's last frame: skipped


def test_candidates_that_offer_nothing(oracle):
    """an all-invalid candidate changes nothing; a full own mask leaves every byte unchanged"""
    rows, cols = 33, 70
    cc = cases.clip_case(oracle.pose_table, rows, cols)
    own = stab.stabilize_frame(cc["images"][1], cc["depths"][1], cc["Rs"][1], cc["ts"][1], cc["K"], cc["M"][1], cc["m"][1])
    assert 0 < own["valid"] < rows * cols
    M, m = spec.neighbour_pose(cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], 1, 2)
    _, _, none_valid = cases.inputs(rows, cols, none_valid=True)
    out, mask, source = own["image"].copy(), own["mask"].copy(), own["mask"].copy()
    assert spec.fill_from(out, mask, source, cc["images"][2], none_valid, cc["Rs"][2], cc["ts"][2], cc["K"], M, m, 3) == 0
    assert np.array_equal(out, own["image"]) and np.array_equal(mask, own["mask"]) and np.array_equal(source, own["mask"])
    out = np.random.default_rng(1).integers(0, 256, size=own["image"].shape, dtype=np.uint8)
    keep, mask, source = out.copy(), np.ones((rows, cols), dtype=np.uint8), np.full((rows, cols), 7, dtype=np.uint8)
    assert spec.fill_from(out, mask, source, cc["images"][2], cc["depths"][2], cc["Rs"][2], cc["ts"][2], cc["K"], M, m, 3) == 0
    assert np.array_equal(out, keep) and mask.all() and (source == 7).all()


# ---------------------------------------------------------------------------------------------------
# the library's host function against the spec
# ---------------------------------------------------------------------------------------------------
def test_library_neighbour_poses_equal_the_spec(rsdsfm):
    p = cases.golden_path()
    A, c, S = p["A"], p["c"], p["scales"]
    for translation in (True, False):
        As, cs = stab.smooth_path(A, c, p["sigma"], translation=translation)
        for radius in (1, 2, 16):
            for q in range(len(S)):
                frames, ids, M, m = rsdsfm.neighbour_poses(A, c, As, cs, S, q, radius)
                order = spec.neighbour_order(q, len(S), radius)
                assert frames.tolist() == order and ids.tolist() == [spec.source_id(n - q) for n in order] and len(order) <= 2 * radius
                for k, n in enumerate(order):
                    wM, wm = spec.neighbour_pose(A, c, As, cs, S, q, n)
                    assert np.allclose(M[k], wM, rtol=0, atol=1e-14) and np.allclose(m[k], wm, rtol=1e-13, atol=1e-300)


def test_host_argument_errors(rsdsfm):
    p = cases.golden_path()
    A, c, S = p["A"], p["c"], p["scales"]
    As, cs = stab.smooth_path(A, c, p["sigma"])
    n = len(S)
    for bad in (dict(q=-1), dict(q=n), dict(radius=0), dict(radius=17), dict(radius=-1)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.neighbour_poses(A, c, As, cs, S, **dict(dict(q=3, radius=2), **bad))
    rsdsfm.neighbour_poses(A, c, As, cs, S, n - 1, 16)
    for bad in (0.0, -1.0, np.nan, np.inf):
        Sb = S.copy()
        Sb[5] = bad
        for q in (3, 4, 6, 7):  # frame 5 is listed
            with pytest.raises(rsdsfm.RsdsfmError):
                rsdsfm.neighbour_poses(A, c, As, cs, Sb, q, 2)
        for q, radius in ((5, 2), (2, 2), (3, 1), (8, 2)):  # the own frame, or not listed: not read
            rsdsfm.neighbour_poses(A, c, As, cs, Sb, q, radius)
    lib = rsdsfm.load_library()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    Af, cf, Asf, csf, Sf = (np.ascontiguousarray(x, dtype=np.float64) for x in (A, c, As, cs, S))
    frames, ids, M, m, k = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32), np.zeros((4, 9)), np.zeros((4, 3)), ctypes.c_int32(-1)
    args = [ptr(Af), ptr(cf), ptr(Asf), ptr(csf), ptr(Sf), ctypes.c_int32(n), ctypes.c_int32(3), ctypes.c_int32(2), ptr(frames), ptr(ids), ptr(M), ptr(m), ctypes.byref(k)]
    assert lib.rsdsfm_neighbour_poses(*args) == rsdsfm.OK and k.value == 4 and frames.tolist() == [2, 4, 1, 5] and ids.tolist() == [2, 3, 4, 5]
    for i in (0, 1, 2, 3, 4, 8, 9, 10, 11, 12):
        assert lib.rsdsfm_neighbour_poses(*[None if j == i else a for j, a in enumerate(args)]) == ERR_INVALID, i
    args[5] = ctypes.c_int32(0)
    assert lib.rsdsfm_neighbour_poses(*args) == ERR_INVALID
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.stabilize_fill_launches(r, c_)
    assert [rsdsfm.stabilize_fill_launches(r, c_) - rsdsfm.rectify_dense_launches(r, c_) for r, c_ in ((2, 2), (300, 400), (720, 1280))] == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------
# golden fixture, accuracy
# ---------------------------------------------------------------------------------------------------
def test_golden_fixture_is_the_spec(oracle):
    """tests/golden/make_golden_stabilize_fill.py wrote the spec's inputs and outputs; recomputed here, so an edit of the spec cannot pass
    unnoticed"""
    assert os.path.getsize(GOLDEN) < 200 * 1024
    g = np.load(GOLDEN)
    names = sorted(set(k.split("/")[0] for k in g.files))
    assert names == ["24x40", "33x70", "5x3"]
    for n in names:
        get = lambda k: g[n + "/" + k]
        q, radius, mode, q5, it = (int(x) for x in get("modes"))
        images, depths = list(get("images")), list(get("depths"))
        rows, cols = depths[0].shape
        cc = cases.clip_case(oracle.pose_table, rows, cols, channels=1 if images[0].ndim == 2 else 3)
        for k, v in (("images", np.stack(cc["images"])), ("depths", np.stack(cc["depths"])), ("R", cc["Rs"][0]), ("t", cc["ts"][0]), ("A", cc["A"]), ("c", cc["c"]),
                     ("A_s", cc["As"]), ("c_s", cc["cs"]), ("scales", cc["scales"]), ("M", cc["M"][q]), ("m", cc["m"][q])):
            assert np.array_equal(get(k), v), (n, k)
        r = spec.stabilize_filled_frame(images, depths, [get("R")] * 4, [get("t")] * 4, tuple(get("K")), get("A"), get("c"), get("A_s"), get("c_s"), get("scales"), q,
                                        get("M"), get("m"), radius=radius, mode=mode, q5_mode=q5, iterations=it)
        for k in ("image", "mask", "source"):
            assert np.array_equal(r[k], get("out_" + k)), (n, k)
        assert r["counts"] == get("out_counts").tolist() and sum(r["counts"]) == rows * cols and len(r["counts"]) == 2 + 2 * radius
    assert g["33x70/out_counts"][2:].sum() > 0 and g["24x40/out_counts"][2:].sum() > 0  # something was filled


def test_accuracy_against_the_analytic_truth(oracle, rsdsfm):
    """two frames of one static scene from two known poses (stabilize_fill_cases.static_scene: tests/test_stabilize_cpu.py's accuracy case as
    the neighbour, a global-shutter frame of the same scene as the own frame, whose virtual camera is turned by 0.05 rad): the band the own
    frame leaves is filled from the neighbour, seen from the own frame's virtual camera.  Truth, independent of stages A and C: the
    neighbour's forward map on the TRUE depth in float64, inverted by 50 fixed-point iterations with synth._bilinear, and the texture evaluated
    analytically there.  Over the filled pixels: mean abs error and position error after 3 iterations below the values measured here on the
    CPU plus half of them (stabilize_fill_cases.ACC_*), and the mean abs error below a tenth of what leaving the band black costs.
    Measured: own 11192 pixels, filled 460, nobody 636; filled mean abs error 0.373208 (max 2.82; the own pixels' 0.3546) against 136.48 black;
    position error 0.072328 px, bound 0.108492."""
    sc = cases.static_scene(rsdsfm.synth, oracle.pose_table)
    r = spec.stabilize_filled_frame(sc["images"], sc["depths"], sc["Rs"], sc["ts"], sc["K"], sc["A"], sc["c"], sc["As"], sc["cs"], sc["scales"], 0, sc["M"], sc["m"],
                                    radius=1, iterations=3)
    filled, own = r["source"] == 3, r["source"] == 1
    assert r["counts"][2] == 0 and r["counts"][3] == int(filled.sum()) > 300 and r["counts"][1] > 0.8 * filled.size
    err = np.abs(r["image"].astype(np.float64) - sc["truth"])
    black = np.abs(sc["truth"])[filled].mean()
    M, m = spec.neighbour_pose(sc["A"], sc["c"], sc["As"], sc["cs"], sc["scales"], 0, 1)
    cand = stab.stabilize_frame(sc["images"][1], sc["depths"][1], sc["Rs"][1], sc["ts"][1], sc["K"], M, m, iterations=3)
    qx, qy = dense.inverse_positions(cand["disp"], 3)
    pos = np.sqrt((qx - sc["px"]) ** 2 + (qy - sc["py"]) ** 2)[filled].max()
    print("counts %s; filled mean abs error %.6f (max %.3f), own %.4f, black %.2f; position error %.6f px (bound %.6f)"
          % (r["counts"], err[filled].mean(), err[filled].max(), err[own].mean(), black, pos, cases.ACC_BOUND))
    assert err[filled].mean() < cases.ACC_MAE_BOUND and err[filled].mean() < 0.1 * black
    assert err[own].mean() < cases.ACC_MAE_BOUND  # the two frames do show one scene
    assert pos < cases.ACC_BOUND


# ---------------------------------------------------------------------------------------------------
# ABI and kernel metadata
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_stabilize_fill_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.stabilize_fill_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    for other in (rsdsfm.declared_symbols(), rsdsfm.video_declared_symbols(), rsdsfm.rectify_video_declared_symbols(), rsdsfm.flow_declared_symbols(),
                  rsdsfm.rectify_dense_declared_symbols(), rsdsfm.flow_check_declared_symbols(), rsdsfm.trajectory_declared_symbols(),
                  rsdsfm.fuse_declared_symbols(), rsdsfm.stabilize_declared_symbols()):
        assert not NEW_SYMBOLS & set(other)
    assert rsdsfm.stabilize_fill_default_params() == dict(radius=spec.RADIUS_DEFAULT) == dict(radius=2)
    assert ctypes.sizeof(rsdsfm.StabilizeFillParams) == 16
    p = rsdsfm.StabilizeFillParams()
    assert lib.rsdsfm_stabilize_fill_params_init(None) != rsdsfm.OK
    assert lib.rsdsfm_stabilize_fill_params_init(ctypes.byref(p)) == rsdsfm.OK and p.radius == 2 and p.struct_bytes == 16 and list(p.reserved) == [0, 0]
    assert os.path.exists(rsdsfm.STABILIZE_FILL_HEADER_PATH)


def test_stabilize_fill_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of stabilize_fill_kernels.hip, its metadata read kernel by kernel (as tests/test_stabilize_cpu.py reads the stabiliser's):
    exactly the two kernels, a zero private segment, no VGPR and no SGPR spills, LDS at most 64 KB"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "stabilize_fill_kernels.hip")
    out = tmp_path / "stabilize_fill_kernels.s"
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
