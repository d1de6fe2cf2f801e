"""GPU-free tests of the retimer (include/rsdsfm_retime.h): the definition (tests/retime_spec_numpy.py) against its golden fixture, the host
functions rsdsfm_path_at and rsdsfm_retime_poses against the definition and against rsdsfm_virtual_poses, the merge's exact cases, the exact
shift scene, the accuracy scene, the exported symbols, the launch counts and the kernel's metadata."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import link_spec_numpy as link  # noqa: E402
import retime_cases as cases  # noqa: E402
import retime_spec_numpy as spec  # noqa: E402
import stabilize_cases as stab_cases  # noqa: E402
import stabilize_spec_numpy as stab  # noqa: E402
from make_golden_retime import digest  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_retime_v1.npz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_retime.h")).read()  # what this file tests is declared there: without the header, nothing here runs
NEW_SYMBOLS = {"rsdsfm_retime_params_init", "rsdsfm_path_at", "rsdsfm_retime_poses", "rsdsfm_retime_merge_dev", "rsdsfm_retime_merge_launches",
               "rsdsfm_retime_frame_dev", "rsdsfm_retime_launches", "rsdsfm_retime_video_dev"}
ERR_INVALID = -1


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
        for k in ("image", "mask", "source"):
            assert np.array_equal(r[k], g[n + k]), (n, k)
        assert list(r["counts"]) == g[n + "counts"].tolist(), n
        seen += np.array(r["counts"])
    assert (seen > 0).all()
    assert os.path.getsize(GOLDEN) <= 256 * 1024
    assert {len(c["images"]) for c in all_cases} == {1, 2} and {c["images"][0].ndim for c in all_cases} == {2, 3}
    assert {(c["occlusion"], c["search"]) for c in all_cases} == {(0, 0), (1, 0), (1, 1)}


def test_the_header_names_its_definition_and_its_symbols():
    assert "tests/retime_spec_numpy.py" in HEADER_TEXT and '#include "rsdsfm_stabilize_search.h"' in HEADER_TEXT
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER_TEXT), name
    assert "d_counts5_or_null" in HEADER_TEXT and "RSDSFM_RETIME_FROM_A 1" in HEADER_TEXT and "NOT here" in HEADER_TEXT


# ---------------------------------------------------------------------------------------------------
# the path between its poses
# ---------------------------------------------------------------------------------------------------
def test_path_at_an_integer_returns_the_entrys_bytes(rsdsfm):
    p = stab_cases.golden_path()
    for q in range(len(p["A"])):
        for fn in (rsdsfm.path_at, spec.path_at):
            A_t, c_t = fn(p["A"], p["c"], float(q))
            assert A_t.tobytes() == np.ascontiguousarray(p["A"][q]).tobytes() and c_t.tobytes() == np.ascontiguousarray(p["c"][q]).tobytes(), q


def test_path_at_the_midpoint_of_a_uniform_path_is_analytic(rsdsfm):
    """a uniform rotation about a fixed axis with a straight walk: the pose at q + tau is exp((q + tau) [w]x), (q + tau) step, to 1e-13; A_t is
    orthonormal to 1e-12; the library is the definition to 1e-15"""
    w, step = np.array([0.004, 0.01, -0.003]), np.array([0.02, -0.01, 0.05])
    A, c = stab_cases.uniform_path(6, w, step)
    for t in (0.5, 2.5, 4.5, 1.25, 3.999, 0.001):
        A_t, c_t = rsdsfm.path_at(A, c, t)
        assert np.abs(A_t - link.rodrigues(t * w)).max() < 1e-13 and np.abs(c_t - t * step).max() < 1e-13, t
        assert np.abs(A_t.T @ A_t - np.eye(3)).max() < 1e-12, t
        A_d, c_d = spec.path_at(A, c, t)
        assert np.abs(A_t - A_d).max() < 1e-15 and np.abs(c_t - c_d).max() < 1e-15, t
    p = stab_cases.golden_path()
    for t in np.random.default_rng(5).uniform(0, len(p["A"]) - 1, size=20):
        A_t, c_t = rsdsfm.path_at(p["A"], p["c"], t)
        A_d, c_d = spec.path_at(p["A"], p["c"], t)
        assert np.abs(A_t.T @ A_t - np.eye(3)).max() < 1e-12
        assert np.abs(A_t - A_d).max() < 1e-15 and np.abs(c_t - c_d).max() < 1e-15, t


def test_path_at_accepts_the_last_pose_and_refuses_outside(rsdsfm):
    A, c = stab_cases.uniform_path(5)
    A_t, c_t = rsdsfm.path_at(A, c, 4.0)
    assert A_t.tobytes() == A[4].tobytes() and c_t.tobytes() == c[4].tobytes()
    rsdsfm.path_at(A[:1], c[:1], 0.0)
    for t in (4.0000001, 5.0, np.nan, np.inf, -1e-9, -1.0):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.path_at(A, c, t)
    lib = rsdsfm.load_library()
    buf = (ctypes.c_double * 9)()
    assert lib.rsdsfm_path_at(None, buf, ctypes.c_int32(1), ctypes.c_double(0.0), buf, buf) == ERR_INVALID
    assert lib.rsdsfm_path_at(buf, buf, ctypes.c_int32(0), ctypes.c_double(0.0), buf, buf) == ERR_INVALID


# ---------------------------------------------------------------------------------------------------
# the sources' poses
# ---------------------------------------------------------------------------------------------------
def test_retime_poses_at_an_integer_is_virtual_poses_entry(rsdsfm):
    """on the smoothed path, bit for bit: the library's two functions share the arithmetic (csrc/stabilize.hpp), and so do the definitions"""
    p = stab_cases.golden_path()
    A, c, S = p["A"], p["c"], p["scales"]
    n = len(S)
    A_s, c_s = rsdsfm.smooth_path(A, c, p["sigma"])
    M, m = rsdsfm.virtual_poses(A, c, A_s, c_s, S)
    Md, md = stab.virtual_poses(A, c, A_s, c_s, S)
    for q in range(n):
        src, w, Mq, mq, A_t, c_t = rsdsfm.retime_poses(A, c, A_s, c_s, S, float(q), nsources=n)
        assert src == (q,) and w == 0 and Mq.shape == (1, 3, 3)
        assert Mq[0].tobytes() == np.ascontiguousarray(M[q]).tobytes() and mq[0].tobytes() == np.ascontiguousarray(m[q]).tobytes(), q
        assert A_t.tobytes() == np.ascontiguousarray(A_s[q]).tobytes()
        d = spec.retime_poses(A, c, A_s, c_s, S, n, float(q))
        assert d["sources"] == (q,) and d["weight"] == 0 and np.array_equal(d["M"][0], Md[q]) and np.array_equal(d["m"][0], md[q])


def test_retime_poses_between_two_frames(rsdsfm):
    p = stab_cases.golden_path()
    A, c, S = p["A"], p["c"], p["scales"]
    n = len(S)
    A_s, c_s = rsdsfm.smooth_path(A, c, p["sigma"])
    for t, weight in ((0.25, 16384), (3.5, 32768), (1e-9, 1), (2 + 1e-9, 1), (1 - 1e-9, 65535), (n - 1 - 1e-9, 65535), (6.75, 49152), (0.3, int(np.rint(0.3 * 65536)))):
        src, w, M, m, A_t, c_t = rsdsfm.retime_poses(A, c, A_s, c_s, S, t, nsources=n)
        q = int(np.floor(t))
        assert src == (q, q + 1) and w == weight and M.shape == (2, 3, 3), t
        d = spec.retime_poses(A, c, A_s, c_s, S, n, t)
        assert d["sources"] == src and d["weight"] == w
        assert np.abs(M - d["M"]).max() < 1e-15 and np.abs(m - d["m"]).max() < 1e-14 and np.abs(A_t - d["A_t"]).max() < 1e-15, t
        for k, s in enumerate(src):  # a point of source s: through the chain's pose into the world, then into the camera at t
            X = np.array([0.3, -0.2, 2.0])
            assert np.abs((M[k] @ X + m[k]) - A_t.T @ (A[s] @ X + (c[s] - c_t) / S[s])).max() < 1e-12
    src, w, M, m, _, _ = rsdsfm.retime_poses(A, c, A, c, S, 2.5, nsources=n)  # the chain itself as the path: an unsmoothed retime
    assert src == (2, 3) and w == 32768


def test_retime_poses_refuses(rsdsfm):
    p = stab_cases.golden_path()
    A, c, S = p["A"], p["c"], p["scales"]
    n = len(S)
    for t in (-0.5, n - 1 + 1e-6, np.nan, np.inf):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.retime_poses(A, c, A, c, S, t, nsources=n)
    with pytest.raises(rsdsfm.RsdsfmError):
        rsdsfm.retime_poses(A, c, A, c, S, 0.0, nsources=0)
    for bad in (0.0, -1.0, np.nan, np.inf):
        Sb = S.copy()
        Sb[3] = bad
        for t in (2.5, 3.0, 3.5):
            with pytest.raises(rsdsfm.RsdsfmError):
                rsdsfm.retime_poses(A, c, A, c, Sb, t, nsources=n)
        rsdsfm.retime_poses(A, c, A, c, Sb, 2.0, nsources=n)  # not a listed source
        rsdsfm.retime_poses(A, c, A, c, Sb, 4.5, nsources=n)
    assert rsdsfm.retime_times(3, 2).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0] and rsdsfm.retime_times(1, 4).tolist() == [0.0]
    assert rsdsfm.retime_times(4, 1).tolist() == [0.0, 1.0, 2.0, 3.0] and len(rsdsfm.retime_times(17, 3)) == 49


# ---------------------------------------------------------------------------------------------------
# the merge
# ---------------------------------------------------------------------------------------------------
def _one(a, b, w, thr=24, ma=1, mb=1):
    """a single gray pixel (in a 2 x 2 frame) through the definition"""
    full = lambda v: np.full((2, 2), v, dtype=np.uint8)
    r = spec.merge(full(a), full(ma), full(b), full(mb), w, thr)
    return int(r["image"][0, 0]), int(r["mask"][0, 0]), int(r["source"][0, 0])


def test_the_merges_exact_cases():
    assert _one(100, 200, 16384, thr=255) == (125, 1, spec.DISSOLVED)
    assert _one(0, 1, 32768) == (1, 1, spec.DISSOLVED) and _one(0, 1, 32767) == (0, 1, spec.DISSOLVED)
    assert _one(100, 124, 1)[2] == spec.DISSOLVED and _one(100, 125, 1)[2] == spec.CONFLICT_A  # d == threshold dissolves, d == threshold + 1 conflicts
    assert _one(100, 110, 1, thr=10)[2] == spec.DISSOLVED and _one(110, 99, 1, thr=10)[2] == spec.CONFLICT_A
    assert _one(10, 200, 32768) == (10, 1, spec.CONFLICT_A) and _one(10, 200, 32769) == (200, 1, spec.CONFLICT_B)
    assert _one(0, 255, 65535, thr=255) == (255, 1, spec.DISSOLVED) and _one(0, 255, 1, thr=255) == (0, 1, spec.DISSOLVED)  # 255 never conflicts
    assert _one(9, 200, 40000, mb=0) == (9, 1, spec.FROM_A) and _one(9, 200, 40000, ma=0) == (200, 1, spec.FROM_B)
    assert _one(9, 200, 40000, ma=0, mb=0) == (0, 0, spec.NONE) and _one(9, 200, 1, ma=77, mb=128)[2] == spec.CONFLICT_A  # any value other than 0 is set
    bgr_a, bgr_b = np.zeros((2, 2, 3), dtype=np.uint8), np.zeros((2, 2, 3), dtype=np.uint8)
    bgr_b[..., 1] = 25  # d is the maximum over the channels
    ones = np.ones((2, 2), dtype=np.uint8)
    assert (spec.merge(bgr_a, ones, bgr_b, ones, 1)["source"] == spec.CONFLICT_A).all()
    bgr_b[..., 1] = 24
    assert (spec.merge(bgr_a, ones, bgr_b, ones, 1)["source"] == spec.DISSOLVED).all()


@pytest.mark.parametrize("shape", cases.MERGE_SHAPES)
@pytest.mark.parametrize("channels", [1, 3])
def test_the_merges_counts_are_the_source_planes_bins(shape, channels):
    ia, ma, ib, mb = cases.merge_layers(*shape, channels)
    a, b = ma != 0, mb != 0
    va, vb = (x.reshape(shape + (-1,)).astype(int) for x in (ia, ib))
    for w in cases.MERGE_WEIGHTS:
        for thr in cases.MERGE_THRESHOLDS:
            r = spec.merge(ia, ma, ib, mb, w, thr)
            bins = np.bincount(r["source"].reshape(-1), minlength=6)
            assert r["counts"] == [bins[0], bins[1], bins[2], bins[3], bins[4] + bins[5]] and sum(r["counts"]) == shape[0] * shape[1]
            assert np.array_equal(r["mask"], (a | b).astype(np.uint8)) and np.array_equal(r["source"] == 0, ~(a | b))
            assert (bins[5] == 0) if w <= 32768 else (bins[4] == 0)
            assert thr < 255 or bins[4] + bins[5] == 0
            out = r["image"].reshape(shape + (-1,)).astype(int)
            assert (out[~(a | b)] == 0).all() and np.array_equal(out[a & ~b], va[a & ~b]) and np.array_equal(out[b & ~a], vb[b & ~a])
            lo, hi = np.minimum(va, vb), np.maximum(va, vb)
            assert ((out >= lo) & (out <= hi))[a & b].all()
    r = spec.merge(ia, ma)  # b absent
    assert set(np.unique(r["source"]).tolist()) <= {0, 1} and r["counts"][2:] == [0, 0, 0] and np.array_equal(r["mask"], a.astype(np.uint8))
    if shape[0] * shape[1] >= 96:
        both = spec.merge(ia, ma, ib, mb, 32769, 24)
        assert all(x > 0 for x in both["counts"])


# ---------------------------------------------------------------------------------------------------
# the frame
# ---------------------------------------------------------------------------------------------------
def test_the_shift_scene_is_exact():
    """constant depth 4, K = (32, 32, 20, 12), 24 x 40, two frames SHIFT = 8 columns apart and consistent: at t = 0.5 layer a is frame 0 moved by
    -4 columns and layer b frame 1 moved by +4, so both show the same bytes where both are set, nothing conflicts, and the bands come from
    the shift alone"""
    case = cases.shift_case()
    rows, cols = 24, 40
    half = cases.SHIFT // 2
    assert np.array_equal(case["images"][1][:, :cols - cases.SHIFT], case["images"][0][:, cases.SHIFT:]) and case["weight"] == 32768
    assert case["c"][1].tolist() == [cases.SHIFT * 4.0 / 32.0, 0.0, 0.0]  # disparity = fx baseline / depth
    r = cases.run_spec(case)
    (la, ka), (lb, kb) = r["layers"]
    a_want, b_want = np.zeros((rows, cols), dtype=np.uint8), np.zeros((rows, cols), dtype=np.uint8)
    a_want[:, :cols - half] = 1  # layer a samples frame 0 at x + half: inside up to column cols - half - 1
    b_want[:, half:] = 1         # layer b samples frame 1 at x - half
    assert np.array_equal(ka, a_want) and np.array_equal(kb, b_want)
    assert np.array_equal(la[:, :cols - half], case["images"][0][:, half:]) and np.array_equal(lb[:, half:], case["images"][1][:, :cols - half])
    both = (ka == 1) & (kb == 1)
    assert np.array_equal(la[both], lb[both])
    assert r["counts"] == [0, half * rows, half * rows, (cols - 2 * half) * rows, 0]
    assert (r["source"][:, :half] == spec.FROM_A).all() and (r["source"][:, cols - half:] == spec.FROM_B).all() and (r["source"][:, half:cols - half] == spec.DISSOLVED).all()
    assert np.array_equal(r["image"][both], la[both]) and np.array_equal(r["image"][:, :half], la[:, :half]) and np.array_equal(r["image"][:, cols - half:], lb[:, cols - half:])
    assert (r["mask"] == 1).all()


def test_accuracy_against_the_analytic_truth(rsdsfm):
    """tests/test_stabilize_cpu.py's accuracy scene (96 x 128, analytic texture, TRUE smooth depth) seen from P0 = identity and P1 = that test's
    (M, m); the truth at t = 0.5 is the texture at the pre-image under the true forward map to rsdsfm_path_at's pose.  On the inner region the
    retimed frame's mean absolute error is below frame 0's left as it is and below the plain average's of the two unwarped frames.  The
    condition is the ordering; the values are printed.
    Measured on the CPU: retimed 0.3582, frame 0 as it is 6.1228, the plain average 3.8744; both layers set on 100.0 % of the inner region (66.8 %
    of the frame), flow up to 9.03 px, every overlapping pixel dissolved (11514) and none in conflict."""
    s = cases.accuracy_scene(rsdsfm.synth)
    inner, truth = s["inner"], s["truth"]
    assert inner.sum() > 0.5 * inner.size
    p = spec.retime_poses(s["A"], s["c"], s["A"], s["c"], s["scales"], 2, 0.5)
    assert p["weight"] == 32768 and p["sources"] == (0, 1)
    r = spec.retime_frame(s["frames"], s["depths"], [s["R"]] * 2, [s["t"]] * 2, s["K"], p["M"], p["m"], p["weight"], iterations=3)
    overlap = ((r["layers"][0][1] == 1) & (r["layers"][1][1] == 1))[inner].mean()
    assert overlap >= 0.5  # the comparison is about the dissolve
    err = lambda img: float(np.abs(np.asarray(img, dtype=np.float64) - truth)[inner].mean())
    e_retimed, e_frame0 = err(r["image"]), err(s["frames"][0])
    e_average = err((s["frames"][0].astype(np.float64) + s["frames"][1].astype(np.float64)) / 2.0)
    print("retimed %.4f, frame 0 as it is %.4f, the plain average %.4f; both layers set on %.1f %% of the inner region (%.1f %% of the frame); flow up to %.2f px; counts %s"
          % (e_retimed, e_frame0, e_average, 100.0 * overlap, 100.0 * inner.mean(), np.sqrt((s["flow"] ** 2).sum(-1)).max(), r["counts"]))
    assert r["mask"][inner].all()
    assert e_retimed < e_frame0 and e_retimed < e_average


def test_every_count_is_exercised_by_the_random_frames():
    """over the 20 random tiny frames of the GPU test every one of the five counts is positive (the spec alone), and so is every render call"""
    total, calls = np.zeros(5, dtype=np.int64), set()
    for seed in range(20):
        case = cases.random_case(seed)
        rows, cols = case["depths"][0].shape
        assert 2 <= rows <= 70 and 2 <= cols <= 70
        total += np.array(cases.run_spec(case)["counts"])
        calls.add((case["occlusion"], case["search"]))
    print("random_case(0..19): [none, a only, b only, dissolved, conflict]", total.tolist())
    assert (total > 0).all() and calls == {(0, 0), (1, 0), (1, 1)}


# ---------------------------------------------------------------------------------------------------
# ABI and kernel metadata
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_retime_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.retime_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    assert NEW_SYMBOLS <= set(rsdsfm.declared_symbols())  # tests/test_capi_symbols.py covers them
    for other in (rsdsfm.video_declared_symbols(), rsdsfm.trajectory_declared_symbols(), rsdsfm.stabilize_declared_symbols(), rsdsfm.stabilize_fill_declared_symbols(),
                  rsdsfm.stabilize_crop_declared_symbols(), rsdsfm.stabilize_blend_declared_symbols(), rsdsfm.stabilize_inpaint_declared_symbols(),
                  rsdsfm.last_frame_declared_symbols(), rsdsfm.stabilize_visible_declared_symbols(), rsdsfm.stabilize_search_declared_symbols()):
        assert not NEW_SYMBOLS & set(other)
    for name in ("retime_merge_dev", "retime_merge", "retime_frame_dev", "retime", "retime_video_dev"):
        assert callable(getattr(rsdsfm.Solver, name))
    for name in ("path_at", "retime_poses", "retime_times", "retime_launches"):
        assert callable(getattr(rsdsfm, name))
    assert os.path.basename(rsdsfm.RETIME_HEADER_PATH) == "rsdsfm_retime.h"
    assert rsdsfm.retime_default_params() == dict(threshold=24, occlusion=0, occlusion_tol_q16=0)
    assert ctypes.sizeof(rsdsfm.RetimeParams) == 32
    assert (rsdsfm.RETIME_NONE, rsdsfm.RETIME_FROM_A, rsdsfm.RETIME_FROM_B, rsdsfm.RETIME_DISSOLVED, rsdsfm.RETIME_CONFLICT_A, rsdsfm.RETIME_CONFLICT_B) == \
        (spec.NONE, spec.FROM_A, spec.FROM_B, spec.DISSOLVED, spec.CONFLICT_A, spec.CONFLICT_B)


def test_evaluate_takes_the_keyword(rsdsfm):
    import inspect

    assert inspect.signature(rsdsfm.evaluate.evaluate_real_sequence).parameters["retime"].default is None
    with pytest.raises(ValueError, match="stabilize"):
        rsdsfm.evaluate.evaluate_real_sequence(None, [], retime=2)


def test_launch_counts_and_host_errors(rsdsfm):
    assert rsdsfm.retime_merge_launches() == 1
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385), (0, 0)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.retime_launches(r, c_)
    for r, c_ in ((2, 2), (37, 67), (96, 128), (720, 1280), (16384, 16384)):
        for nsrc in (1, 2):
            assert rsdsfm.retime_launches(r, c_, nsrc) == nsrc * rsdsfm.stabilize_window_launches(r, c_) + 1
        for nsrc in (0, 3, -1):
            with pytest.raises(rsdsfm.RsdsfmError):
                rsdsfm.retime_launches(r, c_, nsrc)
    lib = rsdsfm.load_library()
    i32, f64 = ctypes.c_int32, ctypes.c_double
    assert lib.rsdsfm_retime_params_init(None) == ERR_INVALID
    assert lib.rsdsfm_retime_merge_dev(None, None, None, None, None, i32(3), i32(8), i32(8), i32(0), i32(24), None, None, None, None) == ERR_INVALID  # no context
    assert lib.rsdsfm_retime_frame_dev(None, None, i32(3), None, None, None, f64(1), f64(1), f64(0), f64(0), i32(8), i32(8), 0, 0, i32(0), i32(1), None, None, i32(0), None,
                                       None, None, None, None, None) == ERR_INVALID
    assert lib.rsdsfm_retime_video_dev(None, None, i32(1), i32(8), i32(8), i32(3), f64(1), f64(1), f64(0), f64(0), None, None, None, None, None, None, None, None, 0, 0,
                                       i32(0), None, i32(1), None, None, None, None, None, None, None, None) == ERR_INVALID


def test_retime_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of retime_kernels.hip, its metadata read kernel by kernel (as tests/test_stabilize_search_cpu.py reads the search's): the one
    kernel in its four instances (gray / BGR, with and without layer b), a zero private segment, no VGPR and no SGPR spills, LDS at most 64 KB"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "retime_kernels.hip")
    out = tmp_path / "retime_kernels.s"
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src,
                        "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    txt = out.read_text()
    entries = re.split(r"\n  - (?=\.)", txt[txt.index("amdhsa.kernels:"):txt.index("amdhsa.target:")])[1:]  # one YAML list item per kernel
    field = lambda e, k: re.search(r"^\s*\.%s:\s+(\S+)\s*$" % k, e, flags=re.M).group(1)
    kernels = {field(e, "name"): tuple(int(field(e, k)) for k in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"))
               for e in entries}
    names = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", open(src).read()))
    assert names == {"retime_merge_kernel"} and len(kernels) == 4, (sorted(kernels), sorted(names))
    assert all("retime_merge_kernel" in n for n in kernels)
    print({n: m for n, m in kernels.items()})
    bad = {n: m for n, m in kernels.items() if m[1:] != (0, 0, 0) or m[0] > 65536}
    assert not bad, bad
