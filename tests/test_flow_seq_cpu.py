"""CPU: the clip ABI (include/rsdsfm_video.h) -- exported by both library builds, its kernels without a private segment or spills, and
synth.render_sequence's two-frame case equal to render_pair."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_video_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.video_declared_symbols()
    assert set(names) == {"rsdsfm_deep_flow_seq_dev", "rsdsfm_deep_flow_seq", "rsdsfm_set_flow_batch", "rsdsfm_solve_video_dev"}
    assert not [n for n in names if not hasattr(lib, n)]


def _kernel_meta(src, tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    out = tmp_path / (os.path.basename(src) + ".s")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src, "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    txt = out.read_text()
    return re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S*flow_\S*kernel\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                      r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", txt)


def test_flow_seq_kernels_have_no_private_segment(tmp_path):
    """every batched flow kernel has a zero private segment and no spills, and the batched SOR needs no more
    VGPRs or LDS than the single-pair one (hipcc -S of both translation units)"""
    csrc = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc")
    seq = {n: (int(lds), int(ps), int(v), int(sp)) for lds, n, ps, v, sp in _kernel_meta(os.path.join(csrc, "flow_seq_kernels.hip"), tmp_path)}
    assert len(seq) == 8 and all("flow_seq_" in n for n in seq), sorted(seq)
    bad = [(n, m) for n, m in seq.items() if m[1] != 0 or m[3] != 0]
    assert not bad, bad
    one = {n: (int(lds), int(ps), int(v), int(sp)) for lds, n, ps, v, sp in _kernel_meta(os.path.join(csrc, "flow_kernels.hip"), tmp_path)}
    sor1 = [m for n, m in one.items() if "flow_sor_kernel" in n]
    sorb = [m for n, m in seq.items() if "flow_seq_sor_kernel" in n]
    assert len(sor1) == len(sorb) == 1
    assert sorb[0][0] <= sor1[0][0] and sorb[0][2] <= sor1[0][2], (sorb, sor1)


def test_render_sequence_of_two_is_render_pair(rsdsfm):
    rows, cols, gamma = 60, 96, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    a, b, flow, mask = rsdsfm.synth.render_pair(rows, cols, K, v, w, k, gamma, seed=11)
    frames, flow2, mask2 = rsdsfm.synth.render_sequence(2, rows, cols, K, v, w, k, gamma, seed=11)
    assert frames.shape == (2, rows, cols, 3) and frames.dtype == np.uint8
    assert np.array_equal(frames[0], a) and np.array_equal(frames[1], b)
    assert np.array_equal(flow, flow2) and np.array_equal(mask, mask2)
    more, _, _ = rsdsfm.synth.render_sequence(4, rows, cols, K, v, w, k, gamma, seed=11)
    assert np.array_equal(more[:2], frames) and not np.array_equal(more[2], more[1])
