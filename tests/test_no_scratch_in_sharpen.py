"""CPU: the sharpen kernel (csrc/sharpen_kernels.hip) must not need SCRATCH memory (a private segment): sharpen_kernel<CH, CURVE> holds its
5 x 8 window, sixteen column sums and twenty-four column minima and maxima in arrays that stay in registers only while every index is a
compile-time constant.  The compiler decides, so the build is checked: hipcc -S of the translation unit with each library build's flags,
.private_segment_fixed_size and .vgpr_spill_count must be 0 and .vgpr_count at most 128 for every instantiation, and there are exactly four of
them: one and three channels x the fixed strength and the curve.  The LDS image (20 x 70 dwords), the strength table and the counters' words
must leave room for four workgroups in a CU's 160 KB.  (The pattern of tests/test_no_scratch_in_noise_curve.py; the kernels' metadata only.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mangled names: sharpen_kernelILi<CH>ELb<CURVE>EE
PATTERN = r"\S*sharpen_kernelILi[13]ELb[01]EE\S*"
INSTANCES = 4


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    cache = {}

    def get(flags):
        key = tuple(flags)
        if key not in cache:
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            if not (os.path.exists(hipcc) or shutil.which(hipcc)):
                pytest.skip("no hipcc")
            out = tmp_path_factory.mktemp("sharpen") / ("sharpen_kernels%d.s" % len(cache))
            src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "sharpen_kernels.hip")
            p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include")] +
                               list(flags) + [src, "-o", str(out)], capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-3000:]
            cache[key] = out.read_text()
        return cache[key]

    return get


@pytest.mark.parametrize("flags", [[], ["-DRSDSFM_FUSED=1"]])
def test_sharpen_kernels_have_no_private_segment(assembly, flags):
    txt = assembly(flags)
    kernels = re.findall(r"\.name:\s+(%s)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)" % PATTERN, txt)
    assert len(kernels) == INSTANCES and len({n for n, _, _, _ in kernels}) == INSTANCES, kernels
    bad = [(n, ps, sp) for n, ps, vg, sp in kernels if int(ps) != 0 or int(sp) != 0]
    assert not bad, bad
    assert all(int(vg) <= 128 for n, ps, vg, sp in kernels), kernels
    assert len(re.findall(r"\.name:\s+\S*kernel\S*\n", txt)) == INSTANCES  # and no kernel beside them
    lds = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:(?!\s+\.name:).*\n)*?\s+\.name:\s+\S*sharpen_kernel\S*\n", txt)  # of the same kernel's record
    assert len(lds) == INSTANCES and all(20 * 70 * 4 <= int(x) and 4 * int(x) <= 160 * 1024 for x in lds), lds  # four workgroups per CU
    print("sharpen kernels (name, private, vgprs, spills):", kernels, "LDS bytes:", lds)
