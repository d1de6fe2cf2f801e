"""CPU: the kernels of the frame solve's direct hand-off (rsdsfm_set_frame_handoff 0) must not need SCRATCH memory (a private segment): the final
stage that leaves block-local inlier lists, the first refinement pass that gathers its inliers from them (every instantiation of its DIRECT
form) and the output pass that now takes a stride.  They run on the context's stream beside other contexts' kernels like the rest of the tail
(tests/test_no_scratch_in_frame_tail.py).  The compiler decides about spills, so the build is checked: hipcc -S of the translation unit,
.private_segment_fixed_size and .vgpr_spill_count must be 0."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# refine_rf_pass_kernel<NP, FIRST, ZSUM, DIRECT> with FIRST and DIRECT set: ILi6ELb1ELb?ELb1E / ILi7ELb1ELb?ELb1E in the mangled name
CASES = [
    ("ransac_kernels", r"\S*ransac_final_kernel\S*", 1),
    ("ransac_kernels", r"\S*ransac_scatter_kernel\S*", 1),
    ("refine_rf_kernels", r"\S*refine_rf_pass_kernelILi[67]ELb1ELb[01]ELb1EE\S*", 4),
    ("refine_kernels", r"\S*refine_finish_claim_kernel\S*", 1),
]


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    cache = {}

    def get(unit):
        if unit not in cache:
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            if not (os.path.exists(hipcc) or shutil.which(hipcc)):
                pytest.skip("no hipcc")
            out = tmp_path_factory.mktemp("handoff") / (unit + ".s")
            src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", unit + ".hip")
            p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src,
                                "-o", str(out)], capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-3000:]
            cache[unit] = out.read_text()
        return cache[unit]

    return get


@pytest.mark.parametrize("unit,pattern,count", CASES)
def test_frame_handoff_kernels_have_no_private_segment(assembly, unit, pattern, count):
    txt = assembly(unit)
    kernels = re.findall(r"\.name:\s+(%s)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)" % pattern, txt)
    assert len(kernels) == count, kernels
    bad = [(n, ps, sp) for n, ps, sp in kernels if int(ps) != 0 or int(sp) != 0]
    assert not bad, bad
