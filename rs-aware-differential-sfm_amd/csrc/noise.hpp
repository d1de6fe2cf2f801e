// noise.hpp -- the noise level (include/rsdsfm_noise.h): what noise_kernels.hip and noise_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_noise.h"
#include "denoise.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

constexpr int kNoiseBins = RSDSFM_NOISE_BINS;
constexpr int kNoiseQuantileDefault = RSDSFM_NOISE_QUANTILE_DEFAULT, kNoiseQuantileMax = RSDSFM_NOISE_QUANTILE_MAX;
constexpr int kNoiseScaleDefault = RSDSFM_NOISE_SCALE_DEFAULT, kNoiseScaleMax = 255;
constexpr int64_t kNoiseMinSamplesDefault = RSDSFM_NOISE_MIN_SAMPLES_DEFAULT;

// DenseWs::d_noise: [histogram: 1024 uint32][record: 4 uint64], whatever the frame's size
inline size_t noise_ws_bytes() { return kNoiseBins * sizeof(uint32_t) + 4 * sizeof(uint64_t); }
struct NoisePlanes {
    uint32_t* hist;
    uint64_t* record;
};
inline NoisePlanes noise_planes(unsigned char* d_noise) {
    return NoisePlanes{reinterpret_cast<uint32_t*>(d_noise), reinterpret_cast<uint64_t*>(d_noise + kNoiseBins * sizeof(uint32_t))};
}

// on c->stream (arguments checked and defaults resolved by the caller): the histogram zeroed by a memset, then the two launches
int noise_level_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, int channels, int rows, int cols, int quantile, unsigned* d_hist,
                       unsigned long long* d_record);

// denoise_accumulate_launch and denoise_spatial_launch (denoise.hpp) with the strength formed from d_noise4 on the device
int denoise_accumulate_auto_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                                   int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int fallback, const unsigned long long* d_noise4,
                                   int scale, int64_t min_samples, uint16_t* d_cells, bool first, bool last, unsigned char* d_image_out, unsigned char* d_mask_out,
                                   unsigned char* d_weight, int64_t* d_counts3);
int denoise_spatial_auto_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, const unsigned char* d_weight, int channels, int rows, int cols, int fallback,
                                const unsigned long long* d_noise4, int scale, int64_t min_samples, int target, int search, unsigned char* d_image_out,
                                unsigned char* d_support, int64_t* d_counts3);

}  // namespace rsdsfm
