"""GPU-free tests of the stabiliser's search for the visible pre-image (include/rsdsfm_stabilize_search.h): the definition
(tests/stabilize_search_spec_numpy.py) against its golden fixture and against the occlusion test's definition it extends, the property it
exists for -- inside a near box's footprint every pixel the occlusion test rejects is recovered from the box --, the constant-depth
identity, the key's tie rule, the exported symbols, the launch count and the kernels' metadata."""
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
import stabilize_search_cases as cases  # noqa: E402
import stabilize_search_spec_numpy as spec  # noqa: E402
import stabilize_visible_cases as vcases  # noqa: E402
import stabilize_visible_spec_numpy as visible  # noqa: E402
from make_golden_stabilize_search import digest  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_stabilize_search_v1.npz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_stabilize_search.h")).read()  # what this file tests is declared there: without the header, nothing here runs
NEW_SYMBOLS = {"rsdsfm_stabilize_search_frame_dev", "rsdsfm_stabilize_search_launches", "rsdsfm_set_occlusion_search"}
KERNELS = {"stabilize_search_map_kernel", "stabilize_search_warp_kernel", "stabilize_search_warp_gray_kernel"}
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


def test_the_header_names_its_definition_and_its_symbols():
    assert "tests/stabilize_search_spec_numpy.py" in HEADER_TEXT and '#include "rsdsfm_stabilize_visible.h"' in HEADER_TEXT
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, HEADER_TEXT), name
    assert "d_counts3_or_null" in HEADER_TEXT and "d_counts2_or_null" not in HEADER_TEXT


def test_the_case_file_has_what_it_promises(oracle):
    names = [c["name"] for c in cases.all_cases(oracle.pose_table)]
    assert names[:-2] == [c["name"] for c in vcases.all_cases(oracle.pose_table)] and names[-2:] == ["two-layer", cases.TIE_CASE]
    for shape in ((24, 40), (37, 67), (16, 131)):
        assert shape in cases.FOLD_SHAPES
    assert {"2x2", "no-valid-depth", "many-to-one", "fold-zoom", "fold-partial-mask"} <= set(names)
    two, once = cases.two_layer_case(), cases.zoom_once_case()
    assert set(np.unique(two["depth"]).tolist()) == {2.0, 4.0, 10.0}
    assert once["iterations"] == 1 and once["window"] == (2, 3, 19, 31) and once["window"] != (0, 0, 24, 40)
    assert cases.run_spec(cases.all_cases(oracle.pose_table)[names.index("no-valid-depth")])["counts"] == (0, 0, 0)  # offers nothing, counts nothing


def test_the_keys_high_word_is_the_z_buffer(oracle):
    """kbuf >> 32 is the occlusion test's zbuf wherever a pixel landed and 0xFFFFFFFF where that holds +inf; D and zv keep their bytes; the low
    word names a source pixel that lands on the cell with exactly that depth, the smallest such index"""
    import rectify_dense_spec_numpy as dense

    landed = 0
    for case in cases.all_cases(oracle.pose_table):
        z = dense.fill_depth(np.asarray(case["depth"], dtype=np.float64))
        args = (z, case["R"], case["t"], *case["K"], case["M"], case["m"], case["mode"], case["q5_mode"])
        D, zv, kbuf = spec.forward_map_keys(*args)
        D0, zv0, zbuf = visible.forward_map_depth(*args)
        assert D.tobytes() == D0.tobytes() and zv.tobytes() == zv0.tobytes() and kbuf.dtype == np.uint64, case["name"]
        high, low = (kbuf >> np.uint64(32)).astype(np.uint32), (kbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)
        empty = zbuf == visible.ZBUF_EMPTY
        assert np.array_equal(high[~empty], zbuf[~empty]) and (high[empty] == 0xFFFFFFFF).all() and (kbuf[empty] == spec.KEY_EMPTY).all(), case["name"]
        assert (low[~empty] < zv.size).all() and np.array_equal(zv.reshape(-1)[low[~empty]].view(np.uint32), zbuf[~empty]), case["name"]
        _, _, klast = spec.forward_map_keys(*args, _largest_index=True)
        assert np.array_equal(klast >> np.uint64(32), kbuf >> np.uint64(32)) and (klast >= kbuf).all(), case["name"]
        landed += int((~empty).sum())
    assert landed > 10000


def _parts(case):
    """the plain window fill, the occlusion test's fill and the search's fill on a case's planes, and the pixels each decision concerns"""
    plain, tested, found = vcases.run_spec(case, visible=False), vcases.run_spec(case), cases.run_spec(case)
    offered = (plain["mask"] == 1) & (case["mask0"] == 0)
    rejected_by_test = offered & (tested["mask"] == 0)
    recovered = (found["mask"] == 1) & (tested["mask"] == 0)
    return plain, tested, found, offered, rejected_by_test, recovered


def test_taken_is_the_tests_taken_and_only_recovered_pixels_differ(oracle):
    """on every case: taken equals the occlusion test's taken, rejected + recovered its rejected; bytes differ from its result only at
    recovered pixels, which get mask 1 and the source id; a rejected pixel keeps what it had"""
    seen = np.zeros(3, dtype=np.int64)
    for case in cases.all_cases(oracle.pose_table):
        plain, tested, found, offered, rejected_by_test, recovered = _parts(case)
        n = case["name"]
        assert found["counts"][0] == tested["counts"][0] and found["counts"][1] + found["counts"][2] == tested["counts"][1], n
        assert found["counts"][2] == int(recovered.sum()) and not (recovered & ~rejected_by_test).any(), n
        for k in ("image", "mask", "source"):
            assert np.array_equal(found[k][~recovered], tested[k][~recovered]), (n, k)
        assert (found["mask"][recovered] == 1).all() and (found["source"][recovered] == cases.SID).all(), n
        still = rejected_by_test & ~recovered
        assert found["counts"][1] == int(still.sum()), n
        assert np.array_equal(found["image"][still], case["image0"][still]) and np.array_equal(found["source"][still], case["source0"][still]), n
        assert (found["mask"][still] == 0).all(), n
        seen += found["counts"]
    assert (seen > 0).all()


@pytest.mark.parametrize("shape", cases.FOLD_SHAPES)
@pytest.mark.parametrize("channels,sign", [(3, 1), (1, -1)])
def test_the_box_is_recovered_inside_its_footprint(shape, channels, sign):
    """the reason for the search: inside the near box's analytic footprint eroded by 2 px, every pixel the occlusion test rejects is recovered,
    from the box (values 160 .. 255), and nothing taken or recovered there is background (values 0 .. 95)"""
    rows, cols = shape
    case = cases.fold_case(rows, cols, channels, sign)
    plain, tested, found, offered, rejected_by_test, recovered = _parts(case)
    r0, r1, c0, c1 = cases.footprint_of(rows, cols, sign, erode=2)
    assert 0 <= r0 < r1 <= rows and 0 <= c0 < c1 <= cols
    inside = np.zeros((rows, cols), dtype=bool)
    inside[r0:r1, c0:c1] = True
    value = found["image"] if found["image"].ndim == 2 else found["image"].min(axis=2)
    rejected_there, recovered_there = int((rejected_by_test & inside).sum()), int((recovered & inside).sum())
    print("%dx%d ch %d sign %+d: rejected by the test %d, recovered %d; inside the eroded footprint rejected %d, recovered %d"
          % (rows, cols, channels, sign, tested["counts"][1], found["counts"][2], rejected_there, recovered_there))
    assert rejected_there >= 1 and recovered_there == rejected_there
    assert np.array_equal(recovered & inside, rejected_by_test & inside)
    assert (value[recovered & inside] >= 160).all()
    written = inside & (found["mask"] == 1) & (case["mask0"] == 0)
    assert not (value[written] < 128).any()


@pytest.mark.parametrize("M,m", [(np.eye(3), np.array([1.0, -0.5, 0.0])), (np.eye(3), np.array([-0.3, 0.2, 0.5])), (stab_cases.M_STD, stab_cases.m_STD)])
@pytest.mark.parametrize("window", [(0, 0, 24, 40), (4, 14, 12, 20)])
def test_constant_depth_searches_nothing(M, m, window):
    """one surface cannot hide itself: on the stabiliser's shift case (constant depth 4) nothing is rejected, nothing is recovered and every
    byte is the window spec's"""
    s = stab_cases.shift_case()
    rng = np.random.default_rng(3)
    mask0 = (rng.random((24, 40)) < 0.3).astype(np.uint8)
    out_a, out_b = (rng.integers(0, 256, size=s["image"].shape, dtype=np.uint8) for _ in range(2))
    out_b[:] = out_a
    mask_a, mask_b, src_a, src_b = mask0.copy(), mask0.copy(), mask0 * 7, mask0 * 7
    taken, rejected, recovered = spec.fill_from_search(out_a, mask_a, src_a, s["image"], s["depth"], s["R"], s["t"], s["K"], M, m, 3, window)
    want = crop.fill_from_window(out_b, mask_b, src_b, s["image"], s["depth"], s["R"], s["t"], s["K"], M, m, 3, window)
    assert rejected == 0 and recovered == 0 and taken == want > 0
    assert np.array_equal(out_a, out_b) and np.array_equal(mask_a, mask_b) and np.array_equal(src_a, src_b)


def test_the_tie_rule_shows_in_the_bytes():
    """where several source pixels of one depth land on one cell the key keeps the SMALLEST index: with the largest instead (the spec's private
    switch) the restart begins elsewhere and, after the case's single iteration, ends elsewhere -- output bytes change.  The case is in the
    golden fixture and in the GPU set, so a kernel with the other rule (or none) fails there"""
    case = cases.zoom_once_case()
    a, b = cases.run_spec(case), cases.run_spec(case, _largest_index=True)
    differ = int((a["image"] != b["image"]).sum())
    print("tie rule: %d output bytes differ, counts %s smallest index, %s largest" % (differ, a["counts"], b["counts"]))
    assert differ >= 1
    assert a["counts"][0] == b["counts"][0]  # the first test does not read the low word


def test_both_outcomes_of_the_search_are_exercised():
    """over the 20 random tiny frames of the GPU test: recovered > 300 and rejected > 100 (the spec alone)"""
    total = np.zeros(3, dtype=np.int64)
    for seed in range(20):
        total += cases.run_spec(cases.random_case(seed))["counts"]
    print("random_case(0..19): taken, rejected, recovered", total.tolist())
    assert total[2] > 300 and total[1] > 100 and total[0] > 1000


# ---------------------------------------------------------------------------------------------------
# ABI and kernel metadata
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_stabilize_search_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.stabilize_search_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    for other in (rsdsfm.declared_symbols(), rsdsfm.video_declared_symbols(), rsdsfm.rectify_video_declared_symbols(), rsdsfm.flow_declared_symbols(),
                  rsdsfm.rectify_dense_declared_symbols(), rsdsfm.flow_check_declared_symbols(), rsdsfm.trajectory_declared_symbols(),
                  rsdsfm.fuse_declared_symbols(), rsdsfm.stabilize_declared_symbols(), rsdsfm.stabilize_fill_declared_symbols(),
                  rsdsfm.stabilize_crop_declared_symbols(), rsdsfm.stabilize_blend_declared_symbols(), rsdsfm.stabilize_inpaint_declared_symbols(),
                  rsdsfm.last_frame_declared_symbols(), rsdsfm.stabilize_visible_declared_symbols()):
        assert not NEW_SYMBOLS & set(other)
    for name in ("stabilize_search_frame_dev", "stabilize_search", "set_occlusion_search"):
        assert callable(getattr(rsdsfm.Solver, name))
    assert os.path.basename(rsdsfm.STABILIZE_SEARCH_HEADER_PATH) == "rsdsfm_stabilize_search.h"


def test_the_clip_wrappers_take_the_keyword(rsdsfm):
    import inspect

    for name in ("stabilize_video_filled_dev", "stabilize_video_cropped_dev", "stabilize_video_blended_dev", "stabilize_video_inpainted_dev"):
        assert inspect.signature(getattr(rsdsfm.Solver, name)).parameters["occlusion_search"].default is False
    assert inspect.signature(rsdsfm.evaluate.evaluate_real_sequence).parameters["occlusion_search"].default is False
    with pytest.raises(ValueError, match="occlusion"):
        rsdsfm.evaluate.evaluate_real_sequence(None, [], occlusion_search=True)


def test_launch_count_and_host_errors(rsdsfm):
    for r, c_ in ((1, 64), (64, 1), (16385, 64), (64, 16385), (0, 0)):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.stabilize_search_launches(r, c_)
    for r, c_ in ((2, 2), (37, 67), (96, 128), (720, 1280), (16384, 16384)):
        assert rsdsfm.stabilize_search_launches(r, c_) == rsdsfm.stabilize_window_launches(r, c_) == rsdsfm.stabilize_visible_launches(r, c_)
    lib = rsdsfm.load_library()
    i32, f64 = ctypes.c_int32, ctypes.c_double
    assert lib.rsdsfm_stabilize_search_frame_dev(None, None, i32(3), None, None, None, f64(1), f64(1), f64(0), f64(0), i32(8), i32(8), 0, 0, i32(0), None, None, i32(2),
                                                 None, None, None, None, i32(0), None) == ERR_INVALID  # no context
    for on in (0, 1, 2):
        assert lib.rsdsfm_set_occlusion_search(None, i32(on)) == ERR_INVALID  # no context


def test_stabilize_search_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of stabilize_search_kernels.hip, its metadata read kernel by kernel (as tests/test_stabilize_visible_cpu.py reads the occlusion
    test's): exactly the three kernels, a zero private segment, no VGPR and no SGPR spills, LDS at most 64 KB"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "stabilize_search_kernels.hip")
    out = tmp_path / "stabilize_search_kernels.s"
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
    print({n: m for n, m in kernels.items()})
    bad = {n: m for n, m in kernels.items() if m[1:] != (0, 0, 0) or m[0] > 65536}
    assert not bad, bad
