"""CPU: the clip rectifier's ABI (include/rsdsfm_rectify_video.h) -- exported by both library builds, every rectifier kernel (the gray
ones among them) without a private segment or spills, and the definition the gray kernels are held to: on a replicated-gray image the
three channels of the oracle's back projection and crack interpolation are equal."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = {"rsdsfm_rectify_gray_frame_dev", "rsdsfm_rectify_video_dev"}
GRAY_KERNELS = {"rectify_claim_gray_kernel", "rectify_write_gray_kernel", "rectify_write_interpolate_gray_kernel", "interpolate_cracky_gray_kernel"}


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_rectify_video_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.rectify_video_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    assert not NEW_SYMBOLS & set(rsdsfm.video_declared_symbols()) and not NEW_SYMBOLS & set(rsdsfm.declared_symbols())


def test_rectifier_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of rectify_kernels.hip: every kernel, BGR and gray, has a zero private segment and no VGPR spills"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "rectify_kernels.hip")
    out = tmp_path / "rectify_kernels.s"
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src,
                        "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    meta = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S*kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                      r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", out.read_text())
    kernels = {n: (int(ps), int(sp)) for _, n, ps, _, sp in meta}
    names = set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", open(src).read()))
    assert len(kernels) == len(names) == 12, (sorted(kernels), sorted(names))  # 8 BGR / depth-image kernels + 4 gray ones
    for g in GRAY_KERNELS:
        assert g in names and any(g in n for n in kernels), g
    bad = {n: m for n, m in kernels.items() if m != (0, 0)}
    assert not bad, bad


def test_gray_is_every_channel_of_the_replicated_image(oracle):
    """the gray rectifier's definition: marker (1, 1, 1), black (norm <= 15) and the neighbour mean are symmetric in the channels, so the
    oracle's outputs for a replicated-gray image carry the same byte in all three channels"""
    rng = np.random.default_rng(5)
    rows, cols = 45, 70
    K = (0.8 * cols, 0.8 * cols, cols / 2.0 - 0.3, rows / 2.0 + 0.2)
    g = rng.integers(16, 256, size=(rows, cols), dtype=np.uint8)
    g[rng.random((rows, cols)) < 0.02] = 1
    dark = rng.random((rows, cols)) < 0.05
    g[dark] = rng.integers(0, 9, size=int(dark.sum()), dtype=np.uint8)
    img = np.repeat(g[:, :, None], 3, axis=2)
    depth = rng.uniform(0.6, 2.5, size=(rows, cols))
    R, t = oracle.pose_table(np.array([0.3, -0.2, 0.1]), np.array([0.02, 0.03, -0.04]), 0.1, 0.9, rows)
    gs, _ = oracle.back_project(img, depth, R.reshape(rows, 9), t, *K)
    assert (gs[:, :, 0] != 0).any() and (gs[:, :, 0] <= 8).any()
    assert np.array_equal(gs[:, :, 0], gs[:, :, 1]) and np.array_equal(gs[:, :, 0], gs[:, :, 2])
    for off in (1, 2, 3):
        fx = oracle.interpolate_cracky(gs, off)
        assert np.array_equal(fx[:, :, 0], fx[:, :, 1]) and np.array_equal(fx[:, :, 0], fx[:, :, 2]), off
        assert not np.array_equal(fx, gs), off
