"""CPU: the spatial top-up's kernel (denoise_spatial_kernel<CH, S>, csrc/denoise_spatial_kernels.hip) must not need SCRATCH memory (a private
segment): a thread holds its four pixels' sums, its row window of 2 S + 4 packed pixels and the column sums in arrays that stay in registers only
while every index is a compile-time constant (the columns of the search are unrolled for that, the rows are a loop).  The compiler decides, so
the build is checked: hipcc -S of the translation unit with each library build's flags, .private_segment_fixed_size and .vgpr_spill_count must
be 0 and .vgpr_count at most 128 for every instantiation (a workgroup of four waves then runs at least four to a SIMD's share), and there are
exactly six of them: one and three channels at search 1, 2 and 3.  (The pattern of tests/test_no_scratch_in_deblur.py; the same metadata keys
only.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mangled names: denoise_spatial_kernelILi<CH>ELi<S>EE
PATTERN = r"\S*denoise_spatial_kernelILi[13]ELi[123]EE\S*"
INSTANCES = 2 * 3


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    cache = {}

    def get(flags):
        key = tuple(flags)
        if key not in cache:
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            if not (os.path.exists(hipcc) or shutil.which(hipcc)):
                pytest.skip("no hipcc")
            out = tmp_path_factory.mktemp("denoise_spatial") / ("denoise_spatial_kernels%d.s" % len(cache))
            src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "denoise_spatial_kernels.hip")
            p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include")] +
                               list(flags) + [src, "-o", str(out)], capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-3000:]
            cache[key] = out.read_text()
        return cache[key]

    return get


@pytest.mark.parametrize("flags", [[], ["-DRSDSFM_FUSED=1"]])
def test_denoise_spatial_kernels_have_no_private_segment(assembly, flags):
    txt = assembly(flags)
    kernels = re.findall(r"\.name:\s+(%s)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)" % PATTERN, txt)
    assert len(kernels) == INSTANCES and len({n for n, _, _, _ in kernels}) == INSTANCES, kernels
    bad = [(n, ps, sp) for n, ps, vg, sp in kernels if int(ps) != 0 or int(sp) != 0]
    assert not bad, bad
    assert all(int(vg) <= 128 for n, ps, vg, sp in kernels), kernels
    assert len(re.findall(r"\.name:\s+\S*denoise_spatial\w*kernel\S*\n", txt)) == INSTANCES  # and no instance beside them
