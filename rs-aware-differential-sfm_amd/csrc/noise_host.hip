// noise_host.hip -- C ABI of the noise level (include/rsdsfm_noise.h; tests/noise_spec_numpy.py is the definition, noise_kernels.hip the
// kernels): the primitive, the strength on the host, the accumulate and the top-up with the strength from a record, the frame call, which
// CALLS the public entry points one after another on planes of the context's dense workspace as rsdsfm_denoise_frame_dev does, and the clip
// call, which calls the frame call per frame.
// The frame call's front and tail and the clip call are denoise_estimated_host.hpp's; what stands here is the estimator's own.
#include "clip_stage_host.hpp"
#include "denoise.hpp"
#include "denoise_estimated_host.hpp"
#include "noise.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {
namespace {

rsdsfm_noise_params noise_defaults() {
    return rsdsfm_noise_params{kNoiseQuantileDefault, kNoiseScaleDefault, (int32_t)sizeof(rsdsfm_noise_params), 0, kNoiseMinSamplesDefault, {0, 0, 0, 0}};
}

// every 0 replaced by its default; false: outside its range
bool noise_words_resolve(int32_t* scale, int64_t* min_samples) {
    if (*scale == 0) *scale = kNoiseScaleDefault;
    if (*min_samples == 0) *min_samples = kNoiseMinSamplesDefault;
    return *scale >= 1 && *scale <= kNoiseScaleMax && *min_samples >= 0;
}

bool quantile_resolve(int32_t* quantile) {
    if (*quantile == 0) *quantile = kNoiseQuantileDefault;
    return *quantile >= 1 && *quantile <= kNoiseQuantileMax;
}

bool noise_params_resolve(const rsdsfm_noise_params* in, rsdsfm_noise_params* out) {
    *out = in ? *in : noise_defaults();
    return struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_noise_params)) && quantile_resolve(&out->quantile_q8) && noise_words_resolve(&out->scale, &out->min_samples);
}

const char* const kNoiseWordsMessage = "scale must be in [1, 255] (0: the default, 12) and min_samples >= 0 (0: 1024)";
const char* const kNoiseParamsMessage =
    "rsdsfm_noise_params: quantile_q8 in [1, 256] or 0, scale in [1, 255] or 0, min_samples >= 0, struct_bytes 0 or sizeof (use rsdsfm_noise_params_init)";

// the auto frame call behind the public function's guard; the clip call runs it per frame
int auto_frame(rsdsfm_ctx* ctx, const EstimatedFrame& a, const rsdsfm_noise_params* noise_or_null) {
    Ctx* c = &ctx->c;
    const char* const stage = "denoise auto frame";
    rsdsfm_noise_params np;
    // resolved here, reported by estimated_checks at its place in the order of checks: np is good only once that call has returned RSDSFM_OK
    const char* const refusal = noise_params_resolve(noise_or_null, &np) ? nullptr : kNoiseParamsMessage;
    NoisePlanes nz{nullptr, nullptr};
    EstimatedFront f{};
    int rc = estimated_checks(ctx, stage, "noise record", a, refusal, &f);
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &f.ws->d_layer, blend_layer_bytes(a.rows, a.cols), "denoise auto frame: no memory for the layer");
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &f.ws->d_denoise, denoise_ws_bytes(a.rows, a.cols), "denoise auto frame: no memory for the reference planes and the cells");
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &f.ws->d_noise, noise_ws_bytes(), "denoise auto frame: no memory for the histogram and the record");
    if (rc == RSDSFM_OK) nz = noise_planes(f.ws->d_noise);
    if (rc == RSDSFM_OK) rc = estimated_render(ctx, stage, a, nz.record, &f);
    if (rc != RSDSFM_OK) return rc;
    const DenoisePlanes& r = f.r;
    const BlendLayer l = blend_layer(f.ws->d_layer, a.rows, a.cols);
    // measure, then accumulate per neighbour
    rc = rsdsfm_noise_level_dev(ctx, r.rimage, r.rmask, a.channels, a.rows, a.cols, np.quantile_q8, nz.hist, f.d_estimate);  // behind the render: the noise the weights compare
    if (rc != RSDSFM_OK) return rc;
    if (a.nsrc == 1) {
        rc = rsdsfm_denoise_accumulate_auto_dev(ctx, r.rimage, r.rmask, nullptr, nullptr, a.channels, a.rows, a.cols, nullptr, f.dp.min_overlap, f.dp.gain_mode, f.dp.strength,
                                                f.d_estimate, np.scale, np.min_samples, nullptr, 1, 1, f.d_image, a.d_mask_out, f.d_weight, a.d_counts6_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    for (int k = 1; k < a.nsrc; ++k) {
        rc = neighbour_step(ctx, "denoise auto frame: zeroing the layer failed", f.dp.occlusion == 1, f.dp.occlusion_tol_q16,
                            source_view(a.d_images, a.d_depths_colmajor, a.d_R_rows9, a.d_t_rows3, k), f.g, a.M + 9 * k, a.m + 3 * k, f.window, r.rimage, r.rsource, l.image, l.mask,
                            l.record);
        if (rc != RSDSFM_OK) return rc;
        rc = rsdsfm_denoise_accumulate_auto_dev(ctx, r.rimage, r.rmask, l.image, l.mask, a.channels, a.rows, a.cols, l.record, f.dp.min_overlap, f.dp.gain_mode, f.dp.strength,
                                                f.d_estimate, np.scale, np.min_samples, r.cells, k == 1, k == a.nsrc - 1, f.d_image, a.d_mask_out, f.d_weight, a.d_counts6_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    if (f.top_up)
        return rsdsfm_denoise_spatial_auto_dev(ctx, f.d_image, a.d_mask_out, f.d_weight, a.channels, a.rows, a.cols, f.sp.strength, f.d_estimate, np.scale, np.min_samples, f.sp.target,
                                               f.sp.search, a.d_image_out, a.d_support_or_null, f.d_counts3);
    return estimated_tail(c, f);
}

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_noise_params_init(rsdsfm_noise_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = noise_defaults();
    return RSDSFM_OK;
}

int rsdsfm_noise_level_launches(void) { return 2; }

int rsdsfm_noise_strength(int64_t n, int64_t m, int32_t scale, int32_t fallback, int64_t min_samples) {
    if (fallback == 0) fallback = kDenoiseStrengthDefault;
    if (n < 0 || m < 0 || fallback < 1 || fallback > kDenoiseStrengthMax || !noise_words_resolve(&scale, &min_samples)) return RSDSFM_ERR_INVALID;
    if (n < min_samples) return fallback;
    if (m >= 4096) return kDenoiseStrengthMax;  // (scale m + 8) >> 4 >= 256 for every scale >= 1: no overflow to think about
    const int64_t h = ((int64_t)scale * m + 8) >> 4;
    return h < 1 ? 1 : h > kDenoiseStrengthMax ? kDenoiseStrengthMax : (int)h;
}

int rsdsfm_denoise_auto_frame_launches(int32_t rows, int32_t cols, int32_t nsrc, int32_t with_spatial) {
    const int n = rsdsfm_denoise_launches(rows, cols, nsrc);
    return n < 0 ? n : n + rsdsfm_noise_level_launches() + (with_spatial ? rsdsfm_denoise_spatial_launches() : 0);
}

int rsdsfm_noise_level_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols, int32_t quantile_q8,
                           uint32_t* d_hist1024_out, uint64_t* d_record4_out) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!quantile_resolve(&quantile_q8)) return stage_fail(c, "noise level", "quantile_q8 must be in [1, 256] (0: the default, 128)");
    const int rc = measure_planes_check(c, "noise level", "record", d_image, d_mask, channels, rows, cols, d_hist1024_out, d_record4_out);
    if (rc != RSDSFM_OK) return rc;
    return noise_level_launch(c, d_image, d_mask, channels, rows, cols, quantile_q8, d_hist1024_out, reinterpret_cast<unsigned long long*>(d_record4_out));
}

int rsdsfm_denoise_accumulate_auto_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image_or_null,
                                       const uint8_t* d_layer_mask_or_null, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                                       int64_t min_overlap, int32_t gain_mode, int32_t strength, const uint64_t* d_noise4, int32_t scale, int64_t min_samples,
                                       uint16_t* d_cells_or_null, int32_t first, int32_t last, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null,
                                       int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "denoise auto accumulate";
    if (min_overlap < 0 || (gain_mode != 0 && gain_mode != 1) || strength < 0 || strength > kDenoiseStrengthMax)
        return stage_fail(c, stage, "min_overlap must be >= 0, gain_mode 0 or 1 and strength in [1, 255] (0: the default, 12)");
    if (!noise_words_resolve(&scale, &min_samples)) return stage_fail(c, stage, kNoiseWordsMessage);
    if (!d_noise4) return stage_fail(c, stage, "the noise record is NULL");
    AccumulateOutputs out{d_image_out, d_mask_out, d_weight_or_null, d_counts3_or_null};
    const int rc = accumulate_check(c, "denoise auto", d_ref_image, d_ref_mask, d_layer_image_or_null, d_layer_mask_or_null, channels, rows, cols, d_cells_or_null,
                                    {d_sums8_or_null, d_noise4}, first, last, &out);
    if (rc != RSDSFM_OK) return rc;
    return denoise_accumulate_auto_launch(c, d_ref_image, d_ref_mask, d_layer_image_or_null, d_layer_mask_or_null, channels, rows, cols,
                                          reinterpret_cast<const unsigned long long*>(d_sums8_or_null), min_overlap ? min_overlap : kMinOverlapDefault, gain_mode,
                                          strength ? strength : kDenoiseStrengthDefault, reinterpret_cast<const unsigned long long*>(d_noise4), scale, min_samples,
                                          d_cells_or_null, first == 1, last == 1, out.image, out.mask, out.weight, out.counts);
}

int rsdsfm_denoise_spatial_auto_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, const uint8_t* d_weight_or_null, int32_t channels, int32_t rows,
                                    int32_t cols, int32_t strength, const uint64_t* d_noise4, int32_t scale, int64_t min_samples, int32_t target, int32_t search,
                                    uint8_t* d_image_out, uint8_t* d_support_or_null, int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "denoise spatial auto";
    if (!spatial_words_resolve(&strength, &target, &search)) return spatial_fail(c, stage, kSpatialWordsMessage);
    if (!noise_words_resolve(&scale, &min_samples)) return stage_fail(c, stage, kNoiseWordsMessage);
    if (const char* what = spatial_planes_refusal(d_image, d_mask, d_weight_or_null, channels, rows, cols, d_image_out, d_support_or_null, d_counts3_or_null))
        return spatial_fail(c, stage, what);
    const int rc = estimate_check(c, stage, "noise record", d_noise4, {d_image_out, d_support_or_null, d_counts3_or_null});
    if (rc != RSDSFM_OK) return rc;
    return denoise_spatial_auto_launch(c, d_image, d_mask, d_weight_or_null, channels, rows, cols, strength, reinterpret_cast<const unsigned long long*>(d_noise4), scale,
                                       min_samples, target, search, d_image_out, d_support_or_null, d_counts3_or_null);
}

int rsdsfm_denoise_auto_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                                  const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                                  int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_denoise_params* params_or_null,
                                  const rsdsfm_noise_params* noise_or_null, const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null,
                                  uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, uint8_t* d_support_or_null, int64_t* d_counts6_or_null,
                                  uint64_t* d_noise4_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    DeviceGuard device_guard_(&ctx->c);
    return auto_frame(ctx, EstimatedFrame{d_images, channels, d_depths_colmajor, d_R_rows9, d_t_rows3, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, nsrc, M, m, params_or_null,
                                          spatial_or_null, window_or_null, d_image_out, d_mask_out, d_weight_or_null, d_support_or_null, d_counts6_or_null, d_noise4_or_null},
                      noise_or_null);
}

int rsdsfm_denoise_auto_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                                  double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                                  const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                                  const rsdsfm_denoise_params* params_or_null, const rsdsfm_noise_params* noise_or_null,
                                  const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images,
                                  uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null, uint8_t* const* d_out_supports_or_null, int64_t* counts_or_null,
                                  uint64_t* noise_records_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    DeviceGuard device_guard_(&ctx->c);
    rsdsfm_noise_params np;
    return estimated_clip(ctx, "denoise auto video",
                          EstimatedClip{d_frames, nsources, rows, cols, channels, fx, fy, cx, cy, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, mode, q5_mode, iterations,
                                        params_or_null, spatial_or_null, window_or_null, d_out_images, d_out_masks, d_out_weights_or_null, d_out_supports_or_null, counts_or_null,
                                        noise_records_or_null},
                          noise_params_resolve(noise_or_null, &np) ? nullptr : kNoiseParamsMessage, 4, [&](const EstimatedFrame& f) { return auto_frame(ctx, f, noise_or_null); });
}

}  // extern "C"
