"""CPU: the DeepFlow front end's host-side contract -- pyramid geometry through the C ABI, the numpy spec's behaviour
(tests/flow_spec_numpy.py, the definition the HIP kernels reproduce bit for bit), the exported symbols of both library builds and
kernels without a private segment."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flow_cases as FC
import flow_spec_numpy as S
from conftest import ROOT


@pytest.mark.parametrize("rows,cols,n,last", [(720, 1280, 67, (26, 44)), (1080, 1920, 74, (26, 46))])
def test_flow_levels_at_video_sizes(rsdsfm, rows, cols, n, last):
    lv = rsdsfm.flow_levels(rows, cols)
    assert len(lv) == n and lv[-1] == last and lv == S.flow_levels(rows, cols)
    if (rows, cols) == (720, 1280):
        assert abs(sum(r * c for r, c in lv) / (rows * cols) - 10.26) < 0.01


def test_flow_levels_small_and_custom(rsdsfm):
    assert rsdsfm.flow_levels(26, 26) == [(26, 26)]  # smaller than min_size / downscale: one level
    assert rsdsfm.flow_levels(2, 2) == [(2, 2)]
    for rows, cols, kw in ((37, 53, {}), (120, 160, dict(downscale=0.8)), (480, 640, dict(min_size=10, downscale=0.5)), (64, 300, dict(min_size=0, downscale=0.7))):
        assert rsdsfm.flow_levels(rows, cols, kw or None) == S.flow_levels(rows, cols, kw.get("downscale", 0.95), kw.get("min_size", 25))


def test_flow_default_params_and_bad_params(rsdsfm):
    assert rsdsfm.flow_default_params() == S.DEFAULTS
    for bad in (dict(downscale=1.0), dict(downscale=0.0), dict(omega=2.0), dict(omega=0.0), dict(fixed_point_iterations=0), dict(sor_iterations=-1),
                dict(alpha=0.0), dict(sigma=float("nan"))):
        with pytest.raises(rsdsfm.RsdsfmError):
            rsdsfm.flow_levels(100, 100, bad)
    with pytest.raises(rsdsfm.RsdsfmError):
        rsdsfm.flow_levels(1, 100)


def test_gray_is_opencvs_integer_formula():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(64, 64, 3), dtype=np.uint8)
    g = S.gray(img)
    b, gg, r = (int(x) for x in img[5, 7])
    assert g[5, 7] == (1868 * b + 9617 * gg + 4899 * r + 8192) >> 14
    i = img.astype(np.int64)
    ref = (1868 * i[..., 0] + 9617 * i[..., 1] + 4899 * i[..., 2] + 8192) >> 14
    assert g.dtype == np.float32 and np.array_equal(g, ref.astype(np.float32))
    # the fixed-point weights are OpenCV's 0.114 / 0.587 / 0.299 in 14 bits
    lin = 0.114 * img[..., 0] + 0.587 * img[..., 1] + 0.299 * img[..., 2]
    assert np.abs(g - lin).max() <= 0.51
    assert np.array_equal(S.gray(img[..., :1]), img[..., 0].astype(np.float32))


def _texture(rows, cols, dx=0.0, dy=0.0, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    x, y = x - dx, y - dy
    f = np.full_like(x, 128.0)
    for o in range(4):
        for _ in range(3):
            th, ph = rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
            f += 30.0 / (o + 1) * np.sin(0.03 * 2 ** o * (np.cos(th) * x + np.sin(th) * y) + ph)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def test_spec_identical_images_give_zero_flow():
    a = _texture(60, 96)
    assert np.all(S.deep_flow(a, a) == 0.0)


def test_spec_recovers_a_subpixel_translation():
    a, b = _texture(96, 128), _texture(96, 128, 0.4, -0.3)
    fl = S.deep_flow(a, b)
    assert np.abs(fl[20:-20, 20:-20] - [0.4, -0.3]).max() < 0.05


def test_flow_levels_never_reach_a_side_of_one(rsdsfm):
    """the pyramid stops before a level with a side below 2, whatever min_size (a 1x1 level made the whole field NaN)"""
    want = [(70, 100), (35, 50), (18, 25), (9, 13), (5, 7), (3, 4), (2, 2)]
    assert S.flow_levels(70, 100, 0.5, 0) == want and rsdsfm.flow_levels(70, 100, dict(min_size=0, downscale=0.5)) == want
    assert S.flow_levels(70, 100, 0.74, 0)[-3:] == [(4, 5), (3, 4), (2, 3)]  # then (1, 2) and (1, 1) before the rule
    assert S.flow_levels(70, 100, 0.3, 0) == [(70, 100), (21, 30), (6, 9), (2, 3)]
    assert S.flow_levels(70, 100, 0.8, 0)[-1] == (2, 2) and S.flow_levels(70, 100, 0.5, 1)[-1] == (2, 2)  # as before the rule
    assert S.flow_levels(2, 40, 0.5, 0) == [(2, 40)]  # the next level would be 1 x 20
    assert S.flow_levels(300, 3, 0.5, 0) == [(300, 3), (150, 2)]
    rng = np.random.default_rng(5)
    for _ in range(300):
        rows, cols = (int(x) for x in rng.integers(2, 400, 2))
        down, min_size = float(rng.uniform(0.05, 0.99)), int(rng.choice([0, 1, 2, 25]))
        lv = S.flow_levels(rows, cols, down, min_size)
        assert lv == rsdsfm.flow_levels(rows, cols, dict(downscale=down, min_size=min_size)), (rows, cols, down, min_size)
        assert min(min(l) for l in lv) >= 2 and all(min(l) > min_size for l in lv[1:]), (rows, cols, down, min_size, lv)


@pytest.mark.parametrize("downscale", [0.3, 0.5, 0.74])
def test_spec_is_finite_when_the_pyramid_runs_to_the_floor(downscale):
    """min_size = 0 with downscale < 0.75 reached a 1x1 level: R1 = 1 / 0, and the field was NaN in 14 000 of 14 000 values"""
    case = FC.BY_ID["min0_down%g" % downscale]
    f = FC.spec(case)
    assert f.shape == (70, 100, 2) and np.isfinite(f).all() and 1.0 < np.abs(f).max() < 4.0


def test_float32_spec_is_the_recorded_one():
    """the float64 option must not move a bit of the float32 path: two cases of test_gpu_flow.py::test_bit_identical_to_spec
    against fields recorded before the option existed (tests/golden/make_golden_flow.py)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_flow_spec_v1.npz"))
    for tag, kw in (("37x53", {}), ("60x96", dict(fixed_point_iterations=2, sor_iterations=7, downscale=0.8))):
        got = S.deep_flow(g["a_" + tag], g["b_" + tag], **kw)
        want = g["flow_" + tag]
        assert want.dtype == np.float32 and got.dtype == np.float64 and np.abs(want).max() > 0.01
        assert np.array_equal(got.view(np.uint64), want.astype(np.float64).view(np.uint64)), tag


def test_case_tables_are_complete():
    """the tables of tests/flow_cases.py hold every case tests/test_gpu_flow_edges.py is meant to run"""
    assert len(FC.CONTENT) == 8 and len(FC.PARAMS) == 17 and len(FC.GEOMETRY) == 10 and len(FC.FULL) == 3 and len(FC.CLIPS) == 6
    a, b = FC.pair(FC.BY_ID["bgr_channels_differ"])
    assert a.shape == (70, 100, 3) and not np.array_equal(a[..., 0], a[..., 1]) and not np.array_equal(a[..., 1], a[..., 2])
    assert {int(x) for x in np.unique(FC.pair(FC.BY_ID["checker_shift2"])[0])} == {0, 255}


@pytest.mark.parametrize("case", FC.ALL + [FC.STILL], ids=lambda c: c.id)
def test_edge_cases_are_finite_in_the_spec(case):
    """a GPU mismatch in tests/test_gpu_flow_edges.py can never be a NaN-payload artefact"""
    assert np.isfinite(FC.spec(case)).all()
    if case.cls == "zero":
        assert not FC.spec(case).view(np.uint64).any()  # every bit zero: no negative zero either
    elif case.id != "black_vs_white":  # a uniform 255 step has no gradient to follow: |flow| < 1e-6
        assert np.abs(FC.spec(case)).max() > 1e-3


@pytest.mark.parametrize("case", FC.CLIPS, ids=lambda c: c.id)
def test_clip_pairs_are_finite_in_the_spec(case):
    for i in (1, 2):
        assert np.isfinite(FC.spec(case, i)).all(), i


# max / mean |float32 spec - float64 spec| in px per class of input, measured with the float64 run as the reference (DESIGN section
# 12, "Accuracy"); the bounds are 4 x these (the cases are seeded: the margin absorbs a change of numpy version or of libm)
F64_MEASURED = {
    "zero": (0.0, 0.0),
    "noise": (7.6e-7, 2.9e-7),
    "smooth": (3.9e-5, 2.5e-5),
    "full": (6.1e-5, 1.7e-7),
    "edges": (3.1e-4, 4.1e-5),
    "sigma16": (7.4e-4, 5.8e-5),
    "far": (2.7e-1, 1.2e-3),  # above 0.05 px: see DESIGN section 12 (208 of 7000 pixels of a field that is itself 18 px off the truth)
}


@pytest.mark.parametrize("case", [c for c in FC.ALL + [FC.STILL] if c.cls is not None], ids=lambda c: c.id)
def test_float32_spec_against_float64(case):
    d = np.abs(FC.spec(case) - FC.spec(case, dtype=np.float64))
    mx, mean = F64_MEASURED[case.cls]
    print("%s (%s): max %.3e mean %.3e px" % (case.id, case.cls, d.max(), d.mean()))
    assert d.max() <= 4.0 * mx and d.mean() <= 4.0 * mean, (d.max(), d.mean())


def test_fuzz_generator_200_cases_finite_in_the_spec():
    """tests/fuzz_flow.py counts a non-finite spec field as a failure and leaves no case out: the first 200 cases of the campaign
    the GPU suite runs a slice of (seed 1) and every pair they compare, in the spec alone"""
    kinds, sides = set(), set()
    for n in range(200):
        case = FC.random_case(n, 1)
        assert 2 <= case.rows <= 200 and 2 <= case.cols <= 200
        kinds.add(case.kind)
        sides.update((case.rows, case.cols))
        fr = FC.frames(case, 3 if n % 2 else 2)
        for p in range(len(fr) - 1):
            assert np.isfinite(S.deep_flow(fr[p], fr[p + 1], **case.params)).all(), (n, p, case)
    assert kinds == set(FC.KINDS) and sides >= set(FC.EDGE_SIDES)


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_flow_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.flow_declared_symbols()
    assert set(names) == {"rsdsfm_flow_default_params", "rsdsfm_flow_levels", "rsdsfm_deep_flow_dev", "rsdsfm_deep_flow"}
    assert not [n for n in names if not hasattr(lib, n)]


def test_flow_kernels_have_no_private_segment(tmp_path):
    """a kernel with scratch hung a queue on the MI355X boxes; every flow kernel must have a zero private segment
    and no spills (hipcc -S of the translation unit)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    out = tmp_path / "flow.s"
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "flow_kernels.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src, "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    txt = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*flow_\S*kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", txt)
    assert len(kernels) == 8, kernels
    bad = [(n, ps, sp) for n, ps, sp in kernels if int(ps) != 0 or int(sp) != 0]
    assert not bad, bad
