"""CPU: the clean plate's median (plate_median_kernel<CH, NL, FLAG>, csrc/plate_kernels.hip) must not need SCRATCH memory (a private segment): its
selection holds up to 15 candidates per channel and pixel pair in an array that a fully unrolled compare-exchange network sorts, which stays in
registers only while every index is a compile-time constant.  The compiler decides, so the build is checked: hipcc -S of the translation unit
with each library build's flags, .private_segment_fixed_size and .vgpr_spill_count must be 0 for every instantiation, and there are 20 of them:
channels 1 / 3, the layer counts 0, 2, 4, 7, 14, with and without the flag.  (The pattern of tests/test_no_scratch_in_lma_operands.py; the
metadata keys only.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mangled names: plate_median_kernelILi<CH>ELi<NL>ELb<FLAG>EE
PATTERN = r"\S*plate_median_kernelILi[13]ELi(?:0|2|4|7|14)ELb[01]EE\S*"
INSTANCES = 2 * 5 * 2


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    cache = {}

    def get(flags):
        key = tuple(flags)
        if key not in cache:
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            if not (os.path.exists(hipcc) or shutil.which(hipcc)):
                pytest.skip("no hipcc")
            out = tmp_path_factory.mktemp("plate") / ("plate_kernels%d.s" % len(cache))
            src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "plate_kernels.hip")
            p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include")] +
                               list(flags) + [src, "-o", str(out)], capture_output=True, text=True, timeout=600)
            assert p.returncode == 0, p.stderr[-3000:]
            cache[key] = out.read_text()
        return cache[key]

    return get


@pytest.mark.parametrize("flags", [[], ["-DRSDSFM_FUSED=1"]])
def test_plate_median_kernels_have_no_private_segment(assembly, flags):
    txt = assembly(flags)
    kernels = re.findall(r"\.name:\s+(%s)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)" % PATTERN, txt)
    assert len(kernels) == INSTANCES and len({n for n, _, _, _ in kernels}) == INSTANCES, kernels
    bad = [(n, ps, sp) for n, ps, vg, sp in kernels if int(ps) != 0 or int(sp) != 0]
    assert not bad, bad
    assert all(int(vg) <= 256 for n, ps, vg, sp in kernels), kernels  # a workgroup of four waves always fits


def test_the_instances_are_the_ones_the_cases_cross():
    import plate_cases as cases

    src = open(os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "plate.hpp")).read()
    sizes = [int(x) for x in re.search(r"kPlateSizes\[\]\s*=\s*\{([^}]*)\}", src).group(1).split(",")]
    assert sizes == cases.INSTANCE_SIZES
    for a in sizes[:-1]:  # the last count of an instance and the first of the next are both tested
        assert a in cases.LAYER_COUNTS and a + 1 in cases.LAYER_COUNTS
    assert sizes[-1] in cases.LAYER_COUNTS and {0, 1, 2, 3, 4, 7, 13, 14} <= set(cases.LAYER_COUNTS)
