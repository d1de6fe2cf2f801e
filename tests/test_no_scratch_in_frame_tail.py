"""CPU: the kernels of the frame solve's short launch tail (rsdsfm_set_frame_tail 0) must not need SCRATCH memory (a private segment): they run
on the lanes of the sequence solve beside other streams' kernels like the refinement's passes do (tests/test_no_scratch_in_refine_rf.py).  The
compiler decides about spills, so the build is checked: hipcc -S of the translation unit, .private_segment_fixed_size and .vgpr_spill_count of
refine_finish_claim_kernel and depth_decide_write_kernel must be 0.  (The first pass of the refinement, which now also builds the start
state, is among the kernels tests/test_no_scratch_in_refine_rf.py checks.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("unit,kernel", [("refine_kernels", "refine_finish_claim_kernel"), ("glue_kernels", "depth_decide_write_kernel")])
def test_frame_tail_kernels_have_no_private_segment(tmp_path, unit, kernel):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    out = tmp_path / (unit + ".s")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", unit + ".hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src, "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    txt = out.read_text()
    kernels = re.findall(r"\.name:\s+(\S*%s\S*)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)" % kernel, txt)
    assert len(kernels) == 1, kernels
    bad = [(n, ps, sp) for n, ps, sp in kernels if int(ps) != 0 or int(sp) != 0]
    assert not bad, bad
