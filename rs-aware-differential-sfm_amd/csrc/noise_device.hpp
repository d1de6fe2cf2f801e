// noise_device.hpp -- what the noise level's kernels share on the device (noise_kernels.hip): the strength the two auto kernels form from a record.
#pragma once

namespace rsdsfm {

// the strength from a noise record [n, m, ...] (tests/noise_spec_numpy.py's noise_strength with its defaults resolved by the host; uniform)
__device__ __forceinline__ unsigned noise_strength_dev(const unsigned long long* __restrict__ noise4, unsigned scale, long long min_samples, unsigned fallback) {
    const unsigned long long n = noise4[0], m = noise4[1] < 4096ull ? noise4[1] : 4096ull;  // from 4096 on h is 255 for every scale: no overflow
    if (n < (unsigned long long)min_samples) return fallback;
    const unsigned long long h = (scale * m + 8u) >> 4;
    return h < 1u ? 1u : h > 255u ? 255u : (unsigned)h;
}

}  // namespace rsdsfm
