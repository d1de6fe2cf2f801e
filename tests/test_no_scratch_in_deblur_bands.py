"""CPU: the kernels of the sharpness transfer per scanline band (deblur_band_sharpness_kernel<CH>, deblur_band_accumulate_kernel<CH, FIRST, LAST>,
csrc/deblur_bands_kernels.hip) must not need SCRATCH memory (a private segment): they are the bodies of csrc/deblur_kernels.hip's kernels
(csrc/deblur_device.hpp, csrc/deblur_sharpness_body.hpp) with three band taus and sixteen row taus in LDS, and the accumulate still holds a
thread's four cells, gained bytes and weights in arrays that stay in registers only while every index is a compile-time constant.  The compiler
decides, so the build is checked: hipcc -S of the translation unit with each library build's flags, .private_segment_fixed_size and
.vgpr_spill_count must be 0 and .vgpr_count at most 128 for every instantiation, and there are exactly 10 of them: the band sharpness kernel for
one and three channels, the band accumulate for both, first or not, last or not.  (The pattern of tests/test_no_scratch_in_deblur.py; the same
metadata keys only.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mangled names: deblur_band_sharpness_kernelILi<CH>EE, deblur_band_accumulate_kernelILi<CH>ELb<FIRST>ELb<LAST>EE
PATTERN = r"\S*deblur_band_(?:sharpness_kernelILi[13]EE|accumulate_kernelILi[13]ELb[01]ELb[01]EE)\S*"
INSTANCES = 2 + 2 * 2 * 2


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    cache = {}

    def get(flags):
        key = tuple(flags)
        if key not in cache:
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            if not (os.path.exists(hipcc) or shutil.which(hipcc)):
                pytest.skip("no hipcc")
            out = tmp_path_factory.mktemp("deblur_bands") / ("deblur_bands_kernels%d.s" % len(cache))
            src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "deblur_bands_kernels.hip")
            p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include")] +
                               list(flags) + [src, "-o", str(out)], capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-3000:]
            cache[key] = out.read_text()
        return cache[key]

    return get


@pytest.mark.parametrize("flags", [[], ["-DRSDSFM_FUSED=1"]])
def test_deblur_band_kernels_have_no_private_segment(assembly, flags):
    txt = assembly(flags)
    kernels = re.findall(r"\.name:\s+(%s)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)" % PATTERN, txt)
    assert len(kernels) == INSTANCES and len({n for n, _, _, _ in kernels}) == INSTANCES, kernels
    bad = [(n, ps, sp) for n, ps, vg, sp in kernels if int(ps) != 0 or int(sp) != 0]
    assert not bad, bad
    assert all(int(vg) <= 128 for n, ps, vg, sp in kernels), kernels
    assert len(re.findall(r"\.name:\s+\S*deblur_\w*kernel\S*\n", txt)) == INSTANCES  # and no instance beside them
