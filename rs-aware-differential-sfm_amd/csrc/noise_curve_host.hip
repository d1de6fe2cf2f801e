// noise_curve_host.hip -- C ABI of the noise curve (include/rsdsfm_noise_curve.h; tests/noise_curve_spec_numpy.py is the definition,
// noise_curve_kernels.hip the kernels): the primitive, the strength table on the host, the accumulate and the top-up with the strength per pixel
// from a curve, the frame call, which CALLS the public entry points one after another on planes of the context's dense workspace as
// rsdsfm_denoise_auto_frame_dev does, and the clip call, which calls the frame call per frame.
// The frame call's front and tail and the clip call are denoise_estimated_host.hpp's; what stands here is the estimator's own.
#include "clip_stage_host.hpp"
#include "denoise.hpp"
#include "denoise_estimated_host.hpp"
#include "noise_curve.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {
namespace {

rsdsfm_noise_curve_params curve_defaults() {
    return rsdsfm_noise_curve_params{kNoiseQuantileDefault,   kNoiseScaleDefault,          (int32_t)sizeof(rsdsfm_noise_curve_params), 0,
                                     kNoiseMinSamplesDefault, kCurveBandMinSamplesDefault, {0, 0, 0, 0}};
}

bool curve_quantile_resolve(int32_t* quantile) {
    if (*quantile == 0) *quantile = kNoiseQuantileDefault;
    return *quantile >= 1 && *quantile <= kNoiseQuantileMax;
}

const char* const kCurveWordsMessage = "scale must be in [1, 255] (0: the default, 12), min_samples >= 0 (0: 1024) and band_min_samples >= 0 (0: 256)";

}  // namespace

bool curve_words_resolve(int32_t* scale, int64_t* min_samples, int64_t* band_min_samples) {
    if (*scale == 0) *scale = kNoiseScaleDefault;
    if (*min_samples == 0) *min_samples = kNoiseMinSamplesDefault;
    if (*band_min_samples == 0) *band_min_samples = kCurveBandMinSamplesDefault;
    return *scale >= 1 && *scale <= kNoiseScaleMax && *min_samples >= 0 && *band_min_samples >= 0;
}

bool curve_params_resolve(const rsdsfm_noise_curve_params* in, rsdsfm_noise_curve_params* out) {
    *out = in ? *in : curve_defaults();
    return struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_noise_curve_params)) && curve_quantile_resolve(&out->quantile_q8) &&
           curve_words_resolve(&out->scale, &out->min_samples, &out->band_min_samples);
}

const char* const kCurveParamsMessage =
    "rsdsfm_noise_curve_params: quantile_q8 in [1, 256] or 0, scale in [1, 255] or 0, min_samples >= 0, band_min_samples >= 0, struct_bytes 0 or sizeof (use "
    "rsdsfm_noise_curve_params_init)";

namespace {

// the curve's frame call behind the public function's guard; the clip call runs it per frame
int curve_frame(rsdsfm_ctx* ctx, const EstimatedFrame& a, const rsdsfm_noise_curve_params* curve_or_null) {
    Ctx* c = &ctx->c;
    const char* const stage = "denoise curve frame";
    rsdsfm_noise_curve_params np;
    // resolved here, reported by estimated_checks at its place in the order of checks: np is good only once that call has returned RSDSFM_OK
    const char* const refusal = curve_params_resolve(curve_or_null, &np) ? nullptr : kCurveParamsMessage;
    NoiseCurvePlanes nz{nullptr, nullptr};
    EstimatedFront f{};
    int rc = estimated_checks(ctx, stage, "noise curve", a, refusal, &f);
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &f.ws->d_layer, blend_layer_bytes(a.rows, a.cols), "denoise curve frame: no memory for the layer");
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &f.ws->d_denoise, denoise_ws_bytes(a.rows, a.cols), "denoise curve frame: no memory for the reference planes and the cells");
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &f.ws->d_noise_curve, noise_curve_ws_bytes(), "denoise curve frame: no memory for the histogram and the curve");
    if (rc == RSDSFM_OK) nz = noise_curve_planes(f.ws->d_noise_curve);
    if (rc == RSDSFM_OK) rc = estimated_render(ctx, stage, a, nz.curve, &f);
    if (rc != RSDSFM_OK) return rc;
    const DenoisePlanes& r = f.r;
    const BlendLayer l = blend_layer(f.ws->d_layer, a.rows, a.cols);
    // measure, then accumulate per neighbour
    rc = rsdsfm_noise_curve_dev(ctx, r.rimage, r.rmask, a.channels, a.rows, a.cols, np.quantile_q8, nz.hist, f.d_estimate);  // behind the render: the noise the weights compare
    if (rc != RSDSFM_OK) return rc;
    if (a.nsrc == 1) {
        rc = rsdsfm_denoise_accumulate_curve_dev(ctx, r.rimage, r.rmask, nullptr, nullptr, a.channels, a.rows, a.cols, nullptr, f.dp.min_overlap, f.dp.gain_mode, f.dp.strength,
                                                 f.d_estimate, np.scale, np.min_samples, np.band_min_samples, nullptr, 1, 1, f.d_image, a.d_mask_out, f.d_weight, a.d_counts6_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    for (int k = 1; k < a.nsrc; ++k) {
        rc = neighbour_step(ctx, "denoise curve frame: zeroing the layer failed", f.dp.occlusion == 1, f.dp.occlusion_tol_q16,
                            source_view(a.d_images, a.d_depths_colmajor, a.d_R_rows9, a.d_t_rows3, k), f.g, a.M + 9 * k, a.m + 3 * k, f.window, r.rimage, r.rsource, l.image, l.mask,
                            l.record);
        if (rc != RSDSFM_OK) return rc;
        rc = rsdsfm_denoise_accumulate_curve_dev(ctx, r.rimage, r.rmask, l.image, l.mask, a.channels, a.rows, a.cols, l.record, f.dp.min_overlap, f.dp.gain_mode, f.dp.strength,
                                                 f.d_estimate, np.scale, np.min_samples, np.band_min_samples, r.cells, k == 1, k == a.nsrc - 1, f.d_image, a.d_mask_out, f.d_weight,
                                                 a.d_counts6_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    if (f.top_up)
        return rsdsfm_denoise_spatial_curve_dev(ctx, f.d_image, a.d_mask_out, f.d_weight, a.channels, a.rows, a.cols, f.sp.strength, f.d_estimate, np.scale, np.min_samples,
                                                np.band_min_samples, f.sp.target, f.sp.search, a.d_image_out, a.d_support_or_null, f.d_counts3);
    return estimated_tail(c, f);
}

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_noise_curve_params_init(rsdsfm_noise_curve_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = curve_defaults();
    return RSDSFM_OK;
}

int rsdsfm_noise_curve_launches(void) { return 2; }

int rsdsfm_noise_curve_strengths(const uint64_t* curve36, int32_t scale, int32_t fallback, int64_t min_samples, int64_t band_min_samples, uint8_t* lut256_out) {
    if (fallback == 0) fallback = kDenoiseStrengthDefault;
    if (!curve36 || !lut256_out || fallback < 1 || fallback > kDenoiseStrengthMax || !curve_words_resolve(&scale, &min_samples, &band_min_samples))
        return RSDSFM_ERR_INVALID;
    unsigned long long rows[kCurveWords];
    for (int i = 0; i < kCurveWords; ++i) rows[i] = curve36[i];
    for (int L = 0; L < 256; ++L) lut256_out[L] = (uint8_t)noise_curve_entry(rows, (unsigned)scale, (unsigned)fallback, min_samples, band_min_samples, L);
    return RSDSFM_OK;
}

int rsdsfm_denoise_curve_frame_launches(int32_t rows, int32_t cols, int32_t nsrc, int32_t with_spatial) {
    const int n = rsdsfm_denoise_launches(rows, cols, nsrc);
    return n < 0 ? n : n + rsdsfm_noise_curve_launches() + (with_spatial ? rsdsfm_denoise_spatial_launches() : 0);
}

int rsdsfm_noise_curve_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols, int32_t quantile_q8,
                           uint32_t* d_hist8192_out, uint64_t* d_curve36_out) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!curve_quantile_resolve(&quantile_q8)) return stage_fail(c, "noise curve", "quantile_q8 must be in [1, 256] (0: the default, 128)");
    const int rc = measure_planes_check(c, "noise curve", "curve", d_image, d_mask, channels, rows, cols, d_hist8192_out, d_curve36_out);
    if (rc != RSDSFM_OK) return rc;
    return noise_curve_launch(c, d_image, d_mask, channels, rows, cols, quantile_q8, d_hist8192_out, reinterpret_cast<unsigned long long*>(d_curve36_out));
}

int rsdsfm_denoise_accumulate_curve_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image_or_null,
                                        const uint8_t* d_layer_mask_or_null, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                                        int64_t min_overlap, int32_t gain_mode, int32_t strength, const uint64_t* d_curve36, int32_t scale, int64_t min_samples,
                                        int64_t band_min_samples, uint16_t* d_cells_or_null, int32_t first, int32_t last, uint8_t* d_image_out, uint8_t* d_mask_out,
                                        uint8_t* d_weight_or_null, int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "denoise curve accumulate";
    if (min_overlap < 0 || (gain_mode != 0 && gain_mode != 1) || strength < 0 || strength > kDenoiseStrengthMax)
        return stage_fail(c, stage, "min_overlap must be >= 0, gain_mode 0 or 1 and strength in [1, 255] (0: the default, 12)");
    if (!curve_words_resolve(&scale, &min_samples, &band_min_samples)) return stage_fail(c, stage, kCurveWordsMessage);
    if (!d_curve36) return stage_fail(c, stage, "the noise curve is NULL");
    AccumulateOutputs out{d_image_out, d_mask_out, d_weight_or_null, d_counts3_or_null};
    const int rc = accumulate_check(c, "denoise curve", d_ref_image, d_ref_mask, d_layer_image_or_null, d_layer_mask_or_null, channels, rows, cols, d_cells_or_null,
                                    {d_sums8_or_null, d_curve36}, first, last, &out);
    if (rc != RSDSFM_OK) return rc;
    return denoise_accumulate_curve_launch(c, d_ref_image, d_ref_mask, d_layer_image_or_null, d_layer_mask_or_null, channels, rows, cols,
                                           reinterpret_cast<const unsigned long long*>(d_sums8_or_null), min_overlap ? min_overlap : kMinOverlapDefault, gain_mode,
                                           strength ? strength : kDenoiseStrengthDefault, reinterpret_cast<const unsigned long long*>(d_curve36), scale, min_samples,
                                           band_min_samples, d_cells_or_null, first == 1, last == 1, out.image, out.mask, out.weight, out.counts);
}

int rsdsfm_denoise_spatial_curve_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, const uint8_t* d_weight_or_null, int32_t channels, int32_t rows,
                                     int32_t cols, int32_t strength, const uint64_t* d_curve36, int32_t scale, int64_t min_samples, int64_t band_min_samples,
                                     int32_t target, int32_t search, uint8_t* d_image_out, uint8_t* d_support_or_null, int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "denoise curve spatial";
    if (!spatial_words_resolve(&strength, &target, &search)) return spatial_fail(c, stage, kSpatialWordsMessage);
    if (!curve_words_resolve(&scale, &min_samples, &band_min_samples)) return stage_fail(c, stage, kCurveWordsMessage);
    if (const char* what = spatial_planes_refusal(d_image, d_mask, d_weight_or_null, channels, rows, cols, d_image_out, d_support_or_null, d_counts3_or_null))
        return spatial_fail(c, stage, what);
    const int rc = estimate_check(c, stage, "noise curve", d_curve36, {d_image_out, d_support_or_null, d_counts3_or_null});
    if (rc != RSDSFM_OK) return rc;
    return denoise_spatial_curve_launch(c, d_image, d_mask, d_weight_or_null, channels, rows, cols, strength, reinterpret_cast<const unsigned long long*>(d_curve36), scale,
                                        min_samples, band_min_samples, target, search, d_image_out, d_support_or_null, d_counts3_or_null);
}

int rsdsfm_denoise_curve_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                                   const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                                   int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_denoise_params* params_or_null,
                                   const rsdsfm_noise_curve_params* curve_or_null, const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null,
                                   uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, uint8_t* d_support_or_null, int64_t* d_counts6_or_null,
                                   uint64_t* d_curve36_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    DeviceGuard device_guard_(&ctx->c);
    return curve_frame(ctx, EstimatedFrame{d_images, channels, d_depths_colmajor, d_R_rows9, d_t_rows3, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, nsrc, M, m, params_or_null,
                                           spatial_or_null, window_or_null, d_image_out, d_mask_out, d_weight_or_null, d_support_or_null, d_counts6_or_null, d_curve36_or_null},
                       curve_or_null);
}

int rsdsfm_denoise_curve_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                                   double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                                   const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                                   const rsdsfm_denoise_params* params_or_null, const rsdsfm_noise_curve_params* curve_or_null,
                                   const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images,
                                   uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null, uint8_t* const* d_out_supports_or_null, int64_t* counts_or_null,
                                   uint64_t* noise_curves_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    DeviceGuard device_guard_(&ctx->c);
    rsdsfm_noise_curve_params np;
    return estimated_clip(ctx, "denoise curve video",
                          EstimatedClip{d_frames, nsources, rows, cols, channels, fx, fy, cx, cy, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, mode, q5_mode, iterations,
                                        params_or_null, spatial_or_null, window_or_null, d_out_images, d_out_masks, d_out_weights_or_null, d_out_supports_or_null, counts_or_null,
                                        noise_curves_or_null},
                          curve_params_resolve(curve_or_null, &np) ? nullptr : kCurveParamsMessage, kCurveWords,
                          [&](const EstimatedFrame& f) { return curve_frame(ctx, f, curve_or_null); });
}

}  // extern "C"
