"""CPU: the DeepFlow front end's host-side contract -- pyramid geometry through the C ABI, the numpy spec's behaviour
(tests/flow_spec_numpy.py, the definition the HIP kernels reproduce bit for bit), the exported symbols of both library builds and
kernels without a private segment."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

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
