"""CPU: the staged forms of the analytic pixel pass (rsdsfm_set_lma_operands 0: ransac_lma_staged_kernel<NC, ERR, STG> and
ransac_lma_staged_own_kernel<ERR, STG>, the operand records in LDS) must not need SCRATCH memory (a private segment): the staging thread holds the next tile's operands
in registers across a tile's arithmetic, on top of what the per-lane form keeps, and the kernels have to stay at four waves per SIMD (128
VGPRs).  The compiler decides about spills, so the build is checked: hipcc -S of the translation unit, .private_segment_fixed_size and
.vgpr_spill_count must be 0 for every staged instantiation.  (The pattern of tests/test_no_scratch_in_frame_handoff.py.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mangled names: ransac_lma_staged_kernelILi<NC>ELb<ERR>ELi<STG>EE, ransac_lma_staged_own_kernelILb<ERR>ELi<STG>EE.  STG 1 (the six operands alone: the
# measurement form) exists for the own-iterate kernels only.
CASES = [
    ([], r"\S*ransac_lma_staged_kernelILi[123]ELb[01]ELi[23]EE\S*", 12),
    ([], r"\S*ransac_lma_staged_own_kernelILb[01]ELi[123]EE\S*", 6),
    (["-DRSDSFM_FUSED=1"], r"\S*ransac_lma_staged_kernelILi[123]ELb[01]ELi[23]EE\S*", 12),
    (["-DRSDSFM_FUSED=1"], r"\S*ransac_lma_staged_own_kernelILb[01]ELi[123]EE\S*", 6),
]


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    cache = {}

    def get(flags):
        key = tuple(flags)
        if key not in cache:
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            if not (os.path.exists(hipcc) or shutil.which(hipcc)):
                pytest.skip("no hipcc")
            out = tmp_path_factory.mktemp("lma_operands") / ("ransac_lma_kernels%d.s" % len(cache))
            src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "ransac_lma_kernels.hip")
            p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include")] +
                               list(flags) + [src, "-o", str(out)], capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-3000:]
            cache[key] = out.read_text()
        return cache[key]

    return get


@pytest.mark.parametrize("flags,pattern,count", CASES)
def test_staged_pixel_pass_kernels_have_no_private_segment(assembly, flags, pattern, count):
    txt = assembly(flags)
    kernels = re.findall(r"\.name:\s+(%s)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)" % pattern, txt)
    assert len(kernels) == count, kernels
    bad = [(n, ps, sp) for n, ps, vg, sp in kernels if int(ps) != 0 or int(sp) != 0]
    assert not bad, bad
    assert all(int(vg) <= 128 for n, ps, vg, sp in kernels), kernels  # four waves per SIMD


def test_switch_is_exported(rsdsfm):
    assert "rsdsfm_set_lma_operands" in rsdsfm.declared_symbols()
    for arith in ("reference", "fused"):
        assert hasattr(rsdsfm.load_library(arith=arith), "rsdsfm_set_lma_operands")
