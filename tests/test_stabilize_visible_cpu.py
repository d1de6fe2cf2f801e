"""GPU-free tests of the stabiliser's occlusion test (include/rsdsfm_stabilize_visible.h): the definition
(tests/stabilize_visible_spec_numpy.py) against its golden fixture, the property it exists for -- inside a near box's footprint the plain fill
paints background pixels and the tested fill paints none --, the constant-depth identity, the ABI of the two words of
rsdsfm_stabilize_fill_params that got names, the exported symbols, the launch count and the kernels' metadata."""
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

import stabilize_cases as stab_cases  # noqa: E402
import stabilize_crop_spec_numpy as crop  # noqa: E402
import stabilize_spec_numpy as stab  # noqa: E402
import stabilize_visible_cases as cases  # noqa: E402
import stabilize_visible_spec_numpy as spec  # noqa: E402
from make_golden_stabilize_visible import digest  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_stabilize_visible_v1.npz")
NEW_SYMBOLS = {"rsdsfm_stabilize_visible_frame_dev", "rsdsfm_stabilize_visible_launches"}
KERNELS = {"stabilize_visible_map_kernel", "stabilize_visible_warp_kernel", "stabilize_visible_warp_gray_kernel"}
ERR_INVALID = -1


# ---------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------
def test_spec_equals_the_golden_fixture(oracle):
    g = np.load(GOLDEN)
    all_cases = cases.all_cases(oracle.pose_table)
    assert {k.split("/")[0] for k in g.files} == {c["name"] for c in all_cases}
    for case in all_cases:
        n = case["name"] + "/"
        assert digest(case) == int(g[n + "digest"]), n
        r = cases.run_spec(case)
        for k in ("image", "mask", "source"):
            assert np.array_equal(r[k], g[n + k]), (n, k)
        assert list(r["counts"]) == g[n + "counts"].tolist(), n
    assert os.path.getsize(GOLDEN) <= 256 * 1024


def test_the_cases_reach_what_they_are_for(oracle):
    by = {c["name"]: c for c in cases.all_cases(oracle.pose_table)}
    got = {n: cases.run_spec(c)["counts"] for n, c in by.items() if not n.startswith("fold-")}
    assert got["no-valid-depth"] == (0, 0)  # offers nothing, counts nothing
    assert (by["holes"]["depth"] == 0).mean() > 0.3 and got["holes"][0] > 0 and got["holes"][1] > 0  # stage A's push runs
    assert not np.array_equal(by["rs-table"]["R"][0], by["rs-table"]["R"][-1])                      # a pose per scanline
    c = by["many-to-one"]
    _, zv, zbuf = spec.forward_map_depth(c["depth"], c["R"], c["t"], *c["K"], c["M"], c["m"])
    cells = int((zbuf != spec.ZBUF_EMPTY).sum())
    assert (zv > 0).sum() == zv.size and cells <= 40 and zv.size // cells >= 60  # hundreds of sources on a few cells: a contended minimum
    assert by["fold-zoom"]["window"] == (2, 3, 32, 57) and by["fold-partial-mask"]["mask0"].any() and not by["fold-partial-mask"]["mask0"].all()
    assert sum(got["2x2"]) == 4


def _footprint_counts(case, r, rows, cols, sign):
    """(background-valued, box-valued) pixels TAKEN inside the box's analytic footprint eroded by 2 px: the box is 160 .. 255, the background 0 .. 95"""
    r0, r1, c0, c1 = cases.footprint_of(rows, cols, sign, erode=2)
    assert 0 <= r0 < r1 <= rows and 0 <= c0 < c1 <= cols
    inside = np.zeros((rows, cols), dtype=bool)
    inside[r0:r1, c0:c1] = True
    value = r["image"] if r["image"].ndim == 2 else r["image"][..., 0]
    taken = inside & (r["mask"] == 1) & (case["mask0"] == 0)
    return int((taken & (value < 128)).sum()), int((taken & (value >= 128)).sum())


@pytest.mark.parametrize("shape", cases.FOLD_SHAPES)
@pytest.mark.parametrize("channels,sign", [(3, 1), (1, -1)])
def test_no_background_inside_the_box(shape, channels, sign):
    """the reason for the test: inside the footprint of the near box the plain fill takes background pixels (the fixed point finds the far
    pre-image of a folded map), the tested fill takes none of them and still takes the box"""
    rows, cols = shape
    case = cases.fold_case(rows, cols, channels, sign)
    plain, tested = cases.run_spec(case, visible=False), cases.run_spec(case)
    bad_plain, _ = _footprint_counts(case, plain, rows, cols, sign)
    bad_tested, kept = _footprint_counts(case, tested, rows, cols, sign)
    print("%dx%d ch %d sign %+d: background pixels inside the box %d plain, %d tested; box pixels kept %d; counts plain %s tested %s"
          % (rows, cols, channels, sign, bad_plain, bad_tested, kept, plain["counts"], tested["counts"]))
    assert bad_plain >= 1
    assert bad_tested == 0
    if shape == (16, 131):
        assert kept >= 1
    # a rejected pixel keeps what it had: image, mask and source differ from the plain fill's only where the plain fill took and the tested did not
    lost = (plain["mask"] == 1) & (tested["mask"] == 0)
    assert tested["counts"][1] == int(lost.sum()) == plain["counts"][0] - tested["counts"][0]
    assert np.array_equal(tested["image"][lost], case["image0"][lost]) and np.array_equal(tested["source"][lost], case["source0"][lost])
    assert np.array_equal(tested["image"][~lost], plain["image"][~lost]) and np.array_equal(tested["source"][~lost], plain["source"][~lost])


@pytest.mark.parametrize("M,m", [(np.eye(3), np.array([1.0, -0.5, 0.0])), (np.eye(3), np.array([-0.3, 0.2, 0.5])), (stab_cases.M_STD, stab_cases.m_STD)])
@pytest.mark.parametrize("window", [(0, 0, 24, 40), (4, 14, 12, 20)])
def test_constant_depth_rejects_nothing(M, m, window):
    """one surface cannot hide itself: on the stabiliser's shift case (constant depth 4) nothing is rejected and every byte is the window
    spec's.  With M = I the depth in the virtual camera is one value: lerp of equal values is exact and zn is that value or +inf"""
    s = stab_cases.shift_case()
    rng = np.random.default_rng(3)
    mask0 = (rng.random((24, 40)) < 0.3).astype(np.uint8)
    out_a, out_b = (rng.integers(0, 256, size=s["image"].shape, dtype=np.uint8) for _ in range(2))
    out_b[:] = out_a
    mask_a, mask_b, src_a, src_b = mask0.copy(), mask0.copy(), mask0 * 7, mask0 * 7
    taken, rejected = spec.fill_from_visible(out_a, mask_a, src_a, s["image"], s["depth"], s["R"], s["t"], s["K"], M, m, 3, window)
    want = crop.fill_from_window(out_b, mask_b, src_b, s["image"], s["depth"], s["R"], s["t"], s["K"], M, m, 3, window)
    assert rejected == 0 and taken == want > 0
    assert np.array_equal(out_a, out_b) and np.array_equal(mask_a, mask_b) and np.array_equal(src_a, src_b)


def test_stage_b_keeps_its_bytes_and_the_planes_are_as_defined():
    """D is stab.forward_map's; zv is the float of the depth in the virtual camera or 0; zbuf holds, per cell, the smallest zv that lands there"""
    c = cases.fold_case(24, 40, 3, 1)
    D, zv, zbuf = spec.forward_map_depth(c["depth"], c["R"], c["t"], *c["K"], c["M"], c["m"])
    gx, gy, D0 = stab.forward_map(c["depth"], c["R"], c["t"], *c["K"], c["M"], c["m"])
    assert D.tobytes() == D0.tobytes() and zv.dtype == np.float32 and zbuf.dtype == np.uint32
    assert set(np.unique(zv).tolist()) == {2.0, 10.0}
    want = np.full((24, 40), np.inf, dtype=np.float32)
    for y in range(24):
        for x in range(40):
            if -0.5 <= gx[y, x] < 39.5 and -0.5 <= gy[y, x] < 23.5:
                iy, ix = min(int(gy[y, x] + 0.5), 23), min(int(gx[y, x] + 0.5), 39)
                want[iy, ix] = min(want[iy, ix], zv[y, x])
    assert np.array_equal(zbuf.view(np.float32), want) and np.isinf(want).any() and (want == 2.0).any()
    z = np.full((24, 40), 4.0)
    _, zv2, zbuf2 = spec.forward_map_depth(z, c["R"], c["t"], *c["K"], np.eye(3), (0.0, 0.0, -5.0))  # behind the virtual camera: no depth, no splat
    assert not zv2.any() and (zbuf2 == spec.ZBUF_EMPTY).all()
    assert spec.tolerance_factor(0) == 1.0 + 3277 / 65536.0 and spec.tolerance_factor(65536) == 2.0


# ---------------------------------------------------------------------------------------------------
# ABI and kernel metadata
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_stabilize_visible_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.stabilize_visible_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    for other in (rsdsfm.declared_symbols(), rsdsfm.video_declared_symbols(), rsdsfm.rectify_video_declared_symbols(), rsdsfm.flow_declared_symbols(),
                  rsdsfm.rectify_dense_declared_symbols(), rsdsfm.flow_check_declared_symbols(), rsdsfm.trajectory_declared_symbols(),
                  rsdsfm.fuse_declared_symbols(), rsdsfm.stabilize_declared_symbols(), rsdsfm.stabilize_fill_declared_symbols(),
                  rsdsfm.stabilize_crop_declared_symbols(), rsdsfm.stabilize_blend_declared_symbols(), rsdsfm.stabilize_inpaint_declared_symbols(),
                  rsdsfm.last_frame_declared_symbols()):
        assert not NEW_SYMBOLS & set(other)
    for name in ("stabilize_visible_frame_dev", "stabilize_visible"):
        assert callable(getattr(rsdsfm.Solver, name))
    assert rsdsfm.OCCLUSION_TOL_Q16_DEFAULT == spec.TOL_Q16_DEFAULT == 3277
    assert re.search(r"#define\s+RSDSFM_OCCLUSION_TOL_Q16_DEFAULT\s+3277\b", open(rsdsfm.STABILIZE_VISIBLE_HEADER_PATH).read())


def test_fill_params_words_have_names(rsdsfm):
    """`occlusion` and `occlusion_tol_q16` are the two words that were `reserved`: same offsets, same size, still answered under the old
    name, 0 from the init call"""
    P = rsdsfm.StabilizeFillParams
    assert ctypes.sizeof(P) == 16 and (P.radius.offset, P.struct_bytes.offset, P.occlusion.offset, P.occlusion_tol_q16.offset) == (0, 4, 8, 12)
    assert P.occlusion.size == 4 and P.occlusion_tol_q16.size == 4
    p = P()
    assert rsdsfm.load_library().rsdsfm_stabilize_fill_params_init(ctypes.byref(p)) == 0
    assert (p.radius, p.struct_bytes, p.occlusion, p.occlusion_tol_q16) == (2, 16, 0, 0) and list(p.reserved) == [0, 0]
    p.occlusion, p.occlusion_tol_q16 = 1, 4000
    assert list(p.reserved) == [1, 4000]
    hdr = open(rsdsfm.STABILIZE_FILL_HEADER_PATH).read()
    assert re.search(r"int32_t\s+occlusion;", hdr) and re.search(r"int32_t\s+occlusion_tol_q16;", hdr) and not re.search(r"int32_t\s+reserved\[2\];", hdr)
    q = rsdsfm._stabilize_fill_params(3, True, 0.25)
    assert (q.radius, q.occlusion, q.occlusion_tol_q16) == (3, 1, 16384)
    assert rsdsfm._stabilize_fill_params(0).reserved == [0, 0] and rsdsfm._stabilize_fill_params(0, True).occlusion_tol_q16 == 0
    assert rsdsfm._occlusion_tol_q16(1.0) == 65536 and rsdsfm._occlusion_tol_q16(1.5) == -1 and rsdsfm._occlusion_tol_q16(0.0) == -1


def test_launch_count_and_host_errors(rsdsfm):
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385), (0, 0)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.stabilize_visible_launches(r, c_)
    for r, c_ in ((2, 2), (37, 67), (96, 128), (720, 1280), (16384, 16384)):
        assert rsdsfm.stabilize_visible_launches(r, c_) == rsdsfm.stabilize_window_launches(r, c_) == rsdsfm.stabilize_fill_launches(r, c_)
    lib = rsdsfm.load_library()
    i32, f64 = ctypes.c_int32, ctypes.c_double
    assert lib.rsdsfm_stabilize_visible_frame_dev(None, None, i32(3), None, None, None, f64(1), f64(1), f64(0), f64(0), i32(8), i32(8), 0, 0, i32(0), None, None, i32(2),
                                                  None, None, None, None, i32(0), None) == ERR_INVALID  # no context


def test_stabilize_visible_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of stabilize_visible_kernels.hip, its metadata read kernel by kernel (as tests/test_stabilize_crop_cpu.py reads the crop's):
    exactly the three kernels, a zero private segment, no VGPR and no SGPR spills, LDS at most 64 KB"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "stabilize_visible_kernels.hip")
    out = tmp_path / "stabilize_visible_kernels.s"
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
