// noise_curve.hpp -- the noise curve (include/rsdsfm_noise_curve.h): what noise_curve_kernels.hip and noise_curve_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_noise_curve.h"
#include "noise.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

constexpr int kCurveBands = RSDSFM_NOISE_CURVE_BANDS, kCurveRows = RSDSFM_NOISE_CURVE_ROWS, kCurveWords = RSDSFM_NOISE_CURVE_WORDS;
constexpr int kCurveHistWords = RSDSFM_NOISE_CURVE_HIST_WORDS;
constexpr int64_t kCurveBandMinSamplesDefault = RSDSFM_NOISE_CURVE_BAND_MIN_SAMPLES_DEFAULT;
// an m from here on gives h = 255 wherever it has a weight (32 * 2^24 >> 9 = 2^20), so the table may clamp it: products stay below 2^38
constexpr unsigned long long kCurveMClamp = 1ull << 24;

// DenseWs::d_noise_curve: [histogram: 8 x 1024 uint32][curve: 36 uint64], whatever the frame's size
inline size_t noise_curve_ws_bytes() { return kCurveHistWords * sizeof(uint32_t) + kCurveWords * sizeof(uint64_t); }
struct NoiseCurvePlanes {
    uint32_t* hist;
    uint64_t* curve;
};
inline NoiseCurvePlanes noise_curve_planes(unsigned char* d) {
    return NoiseCurvePlanes{reinterpret_cast<uint32_t*>(d), reinterpret_cast<uint64_t*>(d + kCurveHistWords * sizeof(uint32_t))};
}

// entry L of the strength table (tests/noise_curve_spec_numpy.py's strengths with its defaults resolved by the caller): the one text the host's
// rsdsfm_noise_curve_strengths and the consumers' kernels run
#if defined(__HIPCC__)
__host__ __device__
#endif
inline unsigned noise_curve_entry(const unsigned long long* curve, unsigned scale, unsigned fallback, long long min_samples, long long band_min_samples, int L) {
    if (curve[4 * kCurveBands] < (unsigned long long)min_samples) return fallback;
    const int lo = L < 16 ? 0 : L >= 240 ? kCurveBands - 1 : (L - 16) >> 5;
    const int hi = L < 16 || L >= 240 ? lo : lo + 1;
    const unsigned long long t = L < 16 || L >= 240 ? 0ull : (unsigned long long)((L - 16) & 31);
    // mfill of lo and of hi: the nearest valid band, the lower one on a tie; row 8's m when no band is valid
    unsigned long long mlo = curve[4 * kCurveBands + 1], mhi = mlo;
    int dlo = 2 * kCurveBands, dhi = 2 * kCurveBands;
    for (int b = 0; b < kCurveBands; ++b) {  // ascending: a strict < keeps the lower band on a tie
        const unsigned long long n = curve[4 * b], m = curve[4 * b + 1];
        if (n < (unsigned long long)band_min_samples) continue;
        const int a = b < lo ? lo - b : b - lo, c = b < hi ? hi - b : b - hi;
        if (a < dlo) dlo = a, mlo = m;
        if (c < dhi) dhi = c, mhi = m;
    }
    mlo = mlo < kCurveMClamp ? mlo : kCurveMClamp;
    mhi = mhi < kCurveMClamp ? mhi : kCurveMClamp;
    const unsigned long long M32 = (32ull - t) * mlo + t * mhi;
    const unsigned long long h = ((unsigned long long)scale * M32 + 256ull) >> 9;
    return h < 1ull ? 1u : h > 255ull ? 255u : (unsigned)h;
}

// the curve's words and its parameter struct (noise_curve_host.hip; the temporal noise curve's frame and clip calls take the same struct): every
// 0 replaced by its default; false: outside its range, or a wrong struct_bytes (kCurveParamsMessage)
bool curve_words_resolve(int32_t* scale, int64_t* min_samples, int64_t* band_min_samples);
bool curve_params_resolve(const rsdsfm_noise_curve_params* in, rsdsfm_noise_curve_params* out);
extern const char* const kCurveParamsMessage;

// on c->stream (arguments checked and defaults resolved by the caller): the histogram zeroed by a memset, then the two launches
int noise_curve_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, int channels, int rows, int cols, int quantile, unsigned* d_hist,
                       unsigned long long* d_curve);

// denoise_accumulate_auto_launch and denoise_spatial_auto_launch (noise.hpp) with the strength per pixel from d_curve36
int denoise_accumulate_curve_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                                    int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int fallback, const unsigned long long* d_curve36,
                                    int scale, int64_t min_samples, int64_t band_min_samples, uint16_t* d_cells, bool first, bool last, unsigned char* d_image_out,
                                    unsigned char* d_mask_out, unsigned char* d_weight, int64_t* d_counts3);
int denoise_spatial_curve_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, const unsigned char* d_weight, int channels, int rows, int cols, int fallback,
                                 const unsigned long long* d_curve36, int scale, int64_t min_samples, int64_t band_min_samples, int target, int search,
                                 unsigned char* d_image_out, unsigned char* d_support, int64_t* d_counts3);

}  // namespace rsdsfm
