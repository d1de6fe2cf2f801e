"""CPU: the colour-consistent plate's kernel (plate_medoid_kernel<3, NL, FLAG>, csrc/plate_medoid_kernels.hip) must not need SCRATCH memory (a
private segment): its selection holds up to 15 packed candidates and their 15 costs per pixel in arrays that stay in registers only while every
index is a compile-time constant.  The compiler decides, so the build is checked: hipcc -S of the translation unit with each library build's
flags, .private_segment_fixed_size and .vgpr_spill_count must be 0 and .vgpr_count at most 256 for every instantiation, and there are exactly 10
of them: three channels, the layer counts 0, 2, 4, 7, 14, with and without the flag -- no gray instance, with one channel the call runs
plate_median_kernel.  (The pattern of tests/test_no_scratch_in_plate.py; the same metadata keys only.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mangled names: plate_medoid_kernelILi3ELi<NL>ELb<FLAG>EE
PATTERN = r"\S*plate_medoid_kernelILi3ELi(?:0|2|4|7|14)ELb[01]EE\S*"
INSTANCES = 5 * 2


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    cache = {}

    def get(flags):
        key = tuple(flags)
        if key not in cache:
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            if not (os.path.exists(hipcc) or shutil.which(hipcc)):
                pytest.skip("no hipcc")
            out = tmp_path_factory.mktemp("plate_medoid") / ("plate_medoid_kernels%d.s" % len(cache))
            src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "plate_medoid_kernels.hip")
            p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include")] +
                               list(flags) + [src, "-o", str(out)], capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-3000:]
            cache[key] = out.read_text()
        return cache[key]

    return get


@pytest.mark.parametrize("flags", [[], ["-DRSDSFM_FUSED=1"]])
def test_plate_medoid_kernels_have_no_private_segment(assembly, flags):
    txt = assembly(flags)
    kernels = re.findall(r"\.name:\s+(%s)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)" % PATTERN, txt)
    assert len(kernels) == INSTANCES and len({n for n, _, _, _ in kernels}) == INSTANCES, kernels
    bad = [(n, ps, sp) for n, ps, vg, sp in kernels if int(ps) != 0 or int(sp) != 0]
    assert not bad, bad
    assert all(int(vg) <= 256 for n, ps, vg, sp in kernels), kernels  # a workgroup of four waves always fits
    assert len(re.findall(r"\.name:\s+\S*plate_medoid_kernel\S*\n", txt)) == INSTANCES  # and no instance beside them: none for one channel


def test_the_instances_are_the_medians():
    src = open(os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "plate_medoid_kernels.hip")).read()
    sizes = [int(x) for x in re.search(r"kPlateSizes\[\]\s*=\s*\{([^}]*)\}", open(os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "plate.hpp")).read()).group(1).split(",")]
    for nl in sizes:
        assert "plate_medoid_kernel<3, %d, false>" % nl in src and "plate_medoid_kernel<3, %d, true>" % nl in src
