// sharpen_host.hip -- C ABI of the sharpen stage (include/rsdsfm_sharpen.h; tests/sharpen_spec_numpy.py is the definition, sharpen_kernels.hip
// the kernel): the two primitives, the frame call, which CALLS the public noise curve and the public curve primitive one after another with the
// histogram and, unless the caller has words for it, the curve in the context's dense workspace, and the clip call, which calls the frame call
// per frame.  A clip here is a list of images: it needs no solved clip, so it is not a clip-walk call (clip_stage_host.hpp).
#include <string>
#include <vector>

#include "clip_stage_host.hpp"
#include "denoise.hpp"
#include "noise_curve.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "sharpen.hpp"

namespace rsdsfm {
namespace {

constexpr int kSharpenFramesMax = 4096;

rsdsfm_sharpen_params sharpen_defaults() {
    return rsdsfm_sharpen_params{kSharpenAmountDefault, kSharpenCoringDefault, kSharpenOvershootDefault, kDenoiseStrengthDefault, (int32_t)sizeof(rsdsfm_sharpen_params),
                                 {0, 0, 0}};
}

rsdsfm_noise_curve_params sharpen_curve_defaults() {
    rsdsfm_noise_curve_params p;
    (void)rsdsfm_noise_curve_params_init(&p);
    return p;
}

// amount_q4, coring_q4 and overshoot are taken raw (0 is a value of each); strength's 0 is replaced by its default; false: outside its range
bool sharpen_words_resolve(int32_t amount_q4, int32_t coring_q4, int32_t overshoot, int32_t* strength) {
    if (*strength == 0) *strength = kDenoiseStrengthDefault;
    return amount_q4 >= 0 && amount_q4 <= kSharpenAmountMax && coring_q4 >= 0 && coring_q4 <= kSharpenCoringMax && overshoot >= 0 && overshoot <= kSharpenOvershootMax &&
           *strength >= 1 && *strength <= kDenoiseStrengthMax;
}

bool sharpen_params_resolve(const rsdsfm_sharpen_params* in, rsdsfm_sharpen_params* out) {
    *out = in ? *in : sharpen_defaults();
    return struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_sharpen_params)) && out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 &&
           sharpen_words_resolve(out->amount_q4, out->coring_q4, out->overshoot, &out->strength);
}

// the curve's words of a frame call: every 0 replaced by its default; false: outside its range or a wrong struct_bytes (noise_curve_host.hip's rule)
bool sharpen_curve_params_resolve(const rsdsfm_noise_curve_params* in, rsdsfm_noise_curve_params* out) {
    *out = in ? *in : sharpen_curve_defaults();
    if (out->quantile_q8 == 0) out->quantile_q8 = kNoiseQuantileDefault;
    if (out->scale == 0) out->scale = kNoiseScaleDefault;
    if (out->min_samples == 0) out->min_samples = kNoiseMinSamplesDefault;
    if (out->band_min_samples == 0) out->band_min_samples = kCurveBandMinSamplesDefault;
    return struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_noise_curve_params)) && out->quantile_q8 >= 1 && out->quantile_q8 <= kNoiseQuantileMax && out->scale >= 1 &&
           out->scale <= kNoiseScaleMax && out->min_samples >= 0 && out->band_min_samples >= 0;
}

bool sharpen_scale_words_resolve(int32_t* scale, int64_t* min_samples, int64_t* band_min_samples) {
    if (*scale == 0) *scale = kNoiseScaleDefault;
    if (*min_samples == 0) *min_samples = kNoiseMinSamplesDefault;
    if (*band_min_samples == 0) *band_min_samples = kCurveBandMinSamplesDefault;
    return *scale >= 1 && *scale <= kNoiseScaleMax && *min_samples >= 0 && *band_min_samples >= 0;
}

const char* const kSharpenWordsMessage = "amount_q4 must be in [0, 64], coring_q4 in [0, 64], overshoot in [0, 255] and strength in [1, 255] (0: the default, 12)";
const char* const kSharpenScaleMessage = "scale must be in [1, 255] (0: the default, 12), min_samples >= 0 (0: 1024) and band_min_samples >= 0 (0: 256)";
const char* const kSharpenParamsMessage =
    "rsdsfm_sharpen_params: amount_q4 in [0, 64], coring_q4 in [0, 64], overshoot in [0, 255], strength in [1, 255] or 0, reserved words 0, struct_bytes 0 or sizeof (use "
    "rsdsfm_sharpen_params_init)";
const char* const kSharpenCurveParamsMessage =
    "rsdsfm_noise_curve_params: quantile_q8 in [1, 256] or 0, scale in [1, 255] or 0, min_samples >= 0, band_min_samples >= 0, struct_bytes 0 or sizeof (use "
    "rsdsfm_noise_curve_params_init)";

// what the primitives refuse about their planes, or NULL; d_curve36: only looked at when `curve`
const char* sharpen_planes_refusal(const uint8_t* d_image, const uint8_t* d_mask, int channels, int rows, int cols, const uint8_t* d_image_out, const int64_t* d_counts4,
                                   bool curve, const uint64_t* d_curve36) {
    if (!frame_size_ok(rows, cols)) return "rows and cols must be in [2, 16384]";
    if (channels != 1 && channels != 3) return "channels must be 1 or 3";
    if (!d_image || !d_mask || !d_image_out) return "null device pointer";
    if (((uintptr_t)d_image | (uintptr_t)d_mask | (uintptr_t)d_image_out) & 3u) return "every plane must be 4-byte aligned";
    if ((uintptr_t)d_counts4 & 7u) return "the counters must be 8-byte aligned";
    const void *o = d_image_out, *n = d_counts4;
    if (o == (const void*)d_image || o == (const void*)d_mask) return "an output may not be an input (the kernel reads a halo: in-place is refused)";
    if (n && (n == (const void*)d_image || n == (const void*)d_mask)) return "an output may not be an input";
    if (n == o) return "the outputs must be distinct";
    if (curve) {
        if (!d_curve36) return "the noise curve is NULL";
        if ((uintptr_t)d_curve36 & 7u) return "the noise curve must be 8-byte aligned";
        if ((const void*)d_curve36 == o || (const void*)d_curve36 == n) return "an output may not be the noise curve";
    }
    return nullptr;
}

int sharpen_fail(Ctx* c, const char* stage, const char* what) { return fail(c, RSDSFM_ERR_INVALID, (std::string(stage) + ": " + what).c_str()); }

// everything rsdsfm_sharpen_frame_dev refuses, in front of anything enqueued or allocated; the resolved parameters on success
int sharpen_frame_check(Ctx* c, const char* stage, const uint8_t* d_image, const uint8_t* d_mask, int channels, int rows, int cols, const rsdsfm_sharpen_params* params,
                        const rsdsfm_noise_curve_params* curve_params, const uint8_t* d_image_out, const int64_t* d_counts4, const uint64_t* d_curve36_or_null,
                        rsdsfm_sharpen_params* sp, rsdsfm_noise_curve_params* np) {
    if (!sharpen_params_resolve(params, sp)) return sharpen_fail(c, stage, kSharpenParamsMessage);
    if (!sharpen_curve_params_resolve(curve_params, np)) return sharpen_fail(c, stage, kSharpenCurveParamsMessage);
    if (const char* what = sharpen_planes_refusal(d_image, d_mask, channels, rows, cols, d_image_out, d_counts4, d_curve36_or_null != nullptr, d_curve36_or_null))
        return sharpen_fail(c, stage, what);
    // the curve is an OUTPUT of the measurement: none of its inputs
    if (d_curve36_or_null && ((const void*)d_curve36_or_null == (const void*)d_image || (const void*)d_curve36_or_null == (const void*)d_mask))
        return sharpen_fail(c, stage, "an output may not be an input");
    return RSDSFM_OK;
}

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_sharpen_params_init(rsdsfm_sharpen_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = sharpen_defaults();
    return RSDSFM_OK;
}

int rsdsfm_sharpen_launches(void) { return 1; }

int rsdsfm_sharpen_frame_launches(void) { return rsdsfm_noise_curve_launches() + rsdsfm_sharpen_launches(); }

int rsdsfm_sharpen_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols, int32_t amount_q4,
                       int32_t coring_q4, int32_t overshoot, int32_t strength, uint8_t* d_image_out, int64_t* d_counts4_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!sharpen_words_resolve(amount_q4, coring_q4, overshoot, &strength)) return sharpen_fail(c, "sharpen", kSharpenWordsMessage);
    if (const char* what = sharpen_planes_refusal(d_image, d_mask, channels, rows, cols, d_image_out, d_counts4_or_null, false, nullptr)) return sharpen_fail(c, "sharpen", what);
    return sharpen_launch(c, d_image, d_mask, channels, rows, cols, amount_q4, coring_q4, overshoot, strength, nullptr, 0, 0, 0, d_image_out, d_counts4_or_null);
}

int rsdsfm_sharpen_curve_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols, int32_t amount_q4,
                             int32_t coring_q4, int32_t overshoot, int32_t strength, const uint64_t* d_curve36, int32_t scale, int64_t min_samples,
                             int64_t band_min_samples, uint8_t* d_image_out, int64_t* d_counts4_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "sharpen curve";
    if (!sharpen_words_resolve(amount_q4, coring_q4, overshoot, &strength)) return sharpen_fail(c, stage, kSharpenWordsMessage);
    if (!sharpen_scale_words_resolve(&scale, &min_samples, &band_min_samples)) return sharpen_fail(c, stage, kSharpenScaleMessage);
    if (const char* what = sharpen_planes_refusal(d_image, d_mask, channels, rows, cols, d_image_out, d_counts4_or_null, true, d_curve36)) return sharpen_fail(c, stage, what);
    return sharpen_launch(c, d_image, d_mask, channels, rows, cols, amount_q4, coring_q4, overshoot, strength, reinterpret_cast<const unsigned long long*>(d_curve36), scale,
                          min_samples, band_min_samples, d_image_out, d_counts4_or_null);
}

int rsdsfm_sharpen_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols,
                             const rsdsfm_sharpen_params* params_or_null, const rsdsfm_noise_curve_params* curve_params_or_null, uint8_t* d_image_out,
                             int64_t* d_counts4_or_null, uint64_t* d_curve36_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "sharpen frame";
    rsdsfm_sharpen_params sp;
    rsdsfm_noise_curve_params np;
    int rc = sharpen_frame_check(c, stage, d_image, d_mask, channels, rows, cols, params_or_null, curve_params_or_null, d_image_out, d_counts4_or_null, d_curve36_or_null, &sp, &np);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);  // a size change releases the plane with the rest
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &ws->d_noise_curve, noise_curve_ws_bytes(), "sharpen frame: no memory for the histogram and the curve");
    if (rc != RSDSFM_OK) return rc;
    const NoiseCurvePlanes nz = noise_curve_planes(ws->d_noise_curve);
    uint64_t* const d_curve = d_curve36_or_null ? d_curve36_or_null : nz.curve;
    // the public entry points themselves, so that they run the code they run alone
    rc = rsdsfm_noise_curve_dev(ctx, d_image, d_mask, channels, rows, cols, np.quantile_q8, nz.hist, d_curve);
    if (rc != RSDSFM_OK) return rc;
    return rsdsfm_sharpen_curve_dev(ctx, d_image, d_mask, channels, rows, cols, sp.amount_q4, sp.coring_q4, sp.overshoot, sp.strength, d_curve, np.scale, np.min_samples,
                                    np.band_min_samples, d_image_out, d_counts4_or_null);
}

int rsdsfm_sharpen_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, const uint8_t* const* d_masks, int32_t nframes, int32_t channels, int32_t rows,
                             int32_t cols, const rsdsfm_sharpen_params* params_or_null, const rsdsfm_noise_curve_params* curve_params_or_null,
                             uint8_t* const* d_out_images, int64_t* counts_or_null, uint64_t* curves_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "sharpen video";
    if (nframes < 1 || nframes > kSharpenFramesMax) return sharpen_fail(c, stage, "nframes must be in [1, 4096]");
    if (!d_images || !d_masks || !d_out_images) return sharpen_fail(c, stage, "null array of frames");
    rsdsfm_sharpen_params sp;
    rsdsfm_noise_curve_params np;
    for (int q = 0; q < nframes; ++q) {  // every frame, in front of the first enqueue
        const int rc = sharpen_frame_check(c, stage, d_images[q], d_masks[q], channels, rows, cols, params_or_null, curve_params_or_null, d_out_images[q], nullptr, nullptr, &sp, &np);
        if (rc != RSDSFM_OK) return rc;
    }
    for (int q = 0; q < nframes; ++q)
        for (int k = 0; k < nframes; ++k) {
            if ((const void*)d_out_images[q] == (const void*)d_images[k] || (const void*)d_out_images[q] == (const void*)d_masks[k])
                return sharpen_fail(c, stage, "an output may not be a frame or a mask of the clip");
            if (k != q && d_out_images[q] == d_out_images[k]) return sharpen_fail(c, stage, "the outputs must be distinct");
        }
    // a frame's 40 device words, [counts: 4][curve: 36], when the caller asks for either: one copy and one wait for both
    constexpr int kWords = kSharpenCounters + kCurveWords;
    const bool wanted = counts_or_null || curves_or_null;
    std::vector<int64_t> host(wanted ? (size_t)kWords * (size_t)nframes : 0);
    DeviceCounts words;
    int rc = words.alloc(c, wanted, (size_t)kWords * (size_t)nframes);
    for (int q = 0; q < nframes && rc == RSDSFM_OK; ++q) {
        int64_t* const d_w = words.at((size_t)kWords * (size_t)q);
        rc = rsdsfm_sharpen_frame_dev(ctx, d_images[q], d_masks[q], channels, rows, cols, params_or_null, curve_params_or_null, d_out_images[q], d_w,
                                      d_w ? reinterpret_cast<uint64_t*>(d_w + kSharpenCounters) : nullptr);
    }
    rc = words.fetch(c, wanted ? host.data() : nullptr, rc);
    if (rc != RSDSFM_OK || !wanted) return rc;
    for (int q = 0; q < nframes; ++q) {
        const int64_t* w = host.data() + (size_t)kWords * (size_t)q;
        for (int k = 0; k < kSharpenCounters && counts_or_null; ++k) counts_or_null[(size_t)kSharpenCounters * (size_t)q + k] = w[k];
        for (int k = 0; k < kCurveWords && curves_or_null; ++k) curves_or_null[(size_t)kCurveWords * (size_t)q + k] = (uint64_t)w[kSharpenCounters + k];
    }
    return RSDSFM_OK;
}

}  // extern "C"
