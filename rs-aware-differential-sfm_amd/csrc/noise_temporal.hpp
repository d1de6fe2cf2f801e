// noise_temporal.hpp -- the temporal noise curve (include/rsdsfm_noise_temporal.h): what noise_temporal_kernels.hip and noise_temporal_host.hip
// share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_noise_temporal.h"
#include "denoise.hpp"
#include "noise_curve.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {

// bin = (kPairBinNum D + 128 N) / (256 N), N = 9 CH: 918 / 256 = 3.586 = 4.047 / 1.128 (tests/noise_temporal_spec_numpy.py)
constexpr unsigned kPairBinNum = 918u;
static_assert(kPairBinNum * 27u * 255u + 128u * 27u < 0xffffffffu / 2u && (kPairBinNum * 27u * 255u + 128u * 27u) / (256u * 27u) < (unsigned)kNoiseBins,
              "the product fits 32 bits and the bin needs no clamp");

// DenseWs::d_noise_temporal: [records: 14 x 8 uint64][layer 0 mask: P][layer 0 image: CH P][layer 1 ...], P = blend_plane_bytes (a multiple of 8,
// so every plane is 4-byte aligned): CH + 1 bytes per pixel and neighbour
inline size_t noise_temporal_records_bytes() { return (size_t)kDenoiseLayersMax * 8 * sizeof(uint64_t); }
inline size_t noise_temporal_ws_bytes(int rows, int cols, int channels, int layers) {
    return noise_temporal_records_bytes() + (size_t)layers * (size_t)(channels + 1) * blend_plane_bytes(rows, cols);
}
struct NoiseTemporalLayer {
    unsigned char *mask, *image;
    uint64_t* record;
};
inline NoiseTemporalLayer noise_temporal_layer(unsigned char* d, int rows, int cols, int channels, int j) {
    const size_t P = blend_plane_bytes(rows, cols);
    unsigned char* const base = d + noise_temporal_records_bytes() + (size_t)j * (size_t)(channels + 1) * P;
    return NoiseTemporalLayer{base, base + P, reinterpret_cast<uint64_t*>(d) + 8 * (size_t)j};
}

// noise_curve_kernels.hip's resolve, launched from noise_temporal_kernels.hip as it is: grid kCurveRows, block kBP; quantile in 1 .. 256
__global__ void noise_curve_resolve_kernel(const unsigned* __restrict__ hist, unsigned quantile, unsigned long long* __restrict__ curve);

// on c->stream (arguments checked and defaults resolved by the caller; d_sums NULL: no gain): the histogram zeroed by a memset when `first`,
// then one launch, which adds to it
int noise_pair_hist_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels, int rows,
                           int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, bool first, unsigned* d_hist);
// one launch of noise_curve_resolve_kernel on c->stream
int noise_curve_resolve_launch(Ctx* c, const unsigned* d_hist, int quantile, unsigned long long* d_curve);

}  // namespace rsdsfm
