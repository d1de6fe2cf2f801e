// noise_temporal_host.hip -- C ABI of the temporal noise curve (include/rsdsfm_noise_temporal.h; tests/noise_temporal_spec_numpy.py is the
// definition, noise_temporal_kernels.hip the kernel): the pair histogram, the resolve alone, the frame call, which CALLS the public entry
// points one after another on planes of the context's dense workspace as rsdsfm_denoise_curve_frame_dev does -- with every neighbour kept on
// a stack of layers, because the curve of all of them is resolved before the first accumulate -- and the clip call, which calls the frame call
// per frame.
// The frame call's front and tail and the clip call are denoise_estimated_host.hpp's; what stands here is the estimator's own.
#include "clip_stage_host.hpp"
#include "denoise.hpp"
#include "denoise_estimated_host.hpp"
#include "noise_curve.hpp"
#include "noise_temporal.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {
namespace {

// what the pair histogram refuses, or NULL
const char* pair_refusal(const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image, const uint8_t* d_layer_mask, int channels, int rows, int cols,
                         const uint64_t* d_sums8, int64_t min_overlap, int gain_mode, int first, const uint32_t* d_hist) {
    if (first != 0 && first != 1) return "first must be 0 or 1";
    if (min_overlap < 0 || (gain_mode != 0 && gain_mode != 1)) return "min_overlap must be >= 0 and gain_mode 0 or 1";
    if (!frame_size_ok(rows, cols)) return "rows and cols must be in [2, 16384]";
    if (channels != 1 && channels != 3) return "channels must be 1 or 3";
    if (!d_ref_image || !d_ref_mask || d_ref_image == d_ref_mask) return "the reference needs its image and its mask";
    if (!d_layer_image || !d_layer_mask) return "the layer needs its image and its mask";
    if (d_layer_image == d_layer_mask || d_layer_image == d_ref_image || d_layer_image == d_ref_mask || d_layer_mask == d_ref_image || d_layer_mask == d_ref_mask)
        return "the reference's and the layer's planes must be distinct";
    if (!d_hist) return "the histogram is NULL";
    if (((uintptr_t)d_ref_image | (uintptr_t)d_ref_mask | (uintptr_t)d_layer_image | (uintptr_t)d_layer_mask) & 3u) return "every plane must be 4-byte aligned";
    if ((uintptr_t)d_hist & 3u) return "the histogram must be 4-byte aligned";
    if ((uintptr_t)d_sums8 & 7u) return "the record must be 8-byte aligned";
    const void* const in[5] = {d_ref_image, d_ref_mask, d_layer_image, d_layer_mask, d_sums8};
    for (const void* p : in)
        if (p == (const void*)d_hist) return "the histogram may not be an input or the record";
    return nullptr;
}

// the workspace's records and a stack of at least `layers` layers of `channels` channels, made when first asked for and again when a call needs
// more bytes than it holds
int temporal_stack(Ctx* c, DenseWs* w, int rows, int cols, int channels, int layers) {
    const size_t bytes = noise_temporal_ws_bytes(rows, cols, channels, layers);
    if (w->d_noise_temporal && w->noise_temporal_bytes < bytes) {  // behind whatever the stream still runs on the smaller stack
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(w->d_noise_temporal);
        w->d_noise_temporal = nullptr;
        w->noise_temporal_bytes = 0;
    }
    if (!w->d_noise_temporal) {
        const int rc = ensure_plane(c, &w->d_noise_temporal, bytes, "denoise temporal frame: no memory for the records and the stack of layers");
        if (rc != RSDSFM_OK) return rc;
        w->noise_temporal_bytes = bytes;
    }
    return RSDSFM_OK;
}

// the temporal frame call behind the public function's guard; the clip call runs it per frame
int temporal_frame(rsdsfm_ctx* ctx, const EstimatedFrame& a, const rsdsfm_noise_curve_params* curve_or_null) {
    Ctx* c = &ctx->c;
    const char* const stage = "denoise temporal frame";
    rsdsfm_noise_curve_params np;
    // resolved here, reported by estimated_checks at its place in the order of checks: np is good only once that call has returned RSDSFM_OK
    const char* const refusal = curve_params_resolve(curve_or_null, &np) ? nullptr : kCurveParamsMessage;
    NoiseCurvePlanes nz{nullptr, nullptr};
    EstimatedFront f{};
    int rc = estimated_checks(ctx, stage, "noise curve", a, refusal, &f);
    // no layer: the neighbours go onto the stack
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &f.ws->d_denoise, denoise_ws_bytes(a.rows, a.cols), "denoise temporal frame: no memory for the reference planes and the cells");
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &f.ws->d_noise_curve, noise_curve_ws_bytes(), "denoise temporal frame: no memory for the histogram and the curve");
    if (rc == RSDSFM_OK && a.nsrc > 1) rc = temporal_stack(c, f.ws, a.rows, a.cols, a.channels, a.nsrc - 1);
    if (rc == RSDSFM_OK) nz = noise_curve_planes(f.ws->d_noise_curve);
    if (rc == RSDSFM_OK) rc = estimated_render(ctx, stage, a, nz.curve, &f);
    if (rc != RSDSFM_OK) return rc;
    const DenoisePlanes& r = f.r;
    for (int k = 1; k < a.nsrc; ++k) {  // every neighbour onto its layer of the stack, its record, its pair histogram
        const NoiseTemporalLayer l = noise_temporal_layer(f.ws->d_noise_temporal, a.rows, a.cols, a.channels, k - 1);
        rc = neighbour_step(ctx, "denoise temporal frame: zeroing the layer failed", f.dp.occlusion == 1, f.dp.occlusion_tol_q16,
                            source_view(a.d_images, a.d_depths_colmajor, a.d_R_rows9, a.d_t_rows3, k), f.g, a.M + 9 * k, a.m + 3 * k, f.window, r.rimage, r.rsource, l.image, l.mask,
                            l.record);
        if (rc != RSDSFM_OK) return rc;
        rc = rsdsfm_noise_pair_hist_dev(ctx, r.rimage, r.rmask, l.image, l.mask, a.channels, a.rows, a.cols, l.record, f.dp.min_overlap, f.dp.gain_mode, k == 1, nz.hist);
        if (rc != RSDSFM_OK) return rc;
    }
    if (a.nsrc == 1) RSDSFM_HIP_CHECK(c, hipMemsetAsync(nz.hist, 0, kCurveHistWords * sizeof(uint32_t), c->stream));  // no neighbour: the empty histogram
    rc = rsdsfm_noise_curve_resolve_dev(ctx, nz.hist, np.quantile_q8, f.d_estimate);  // behind every neighbour, in front of the first accumulate
    if (rc != RSDSFM_OK) return rc;
    if (a.nsrc == 1) {
        rc = rsdsfm_denoise_accumulate_curve_dev(ctx, r.rimage, r.rmask, nullptr, nullptr, a.channels, a.rows, a.cols, nullptr, f.dp.min_overlap, f.dp.gain_mode, f.dp.strength,
                                                 f.d_estimate, np.scale, np.min_samples, np.band_min_samples, nullptr, 1, 1, f.d_image, a.d_mask_out, f.d_weight, a.d_counts6_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    for (int k = 1; k < a.nsrc; ++k) {
        const NoiseTemporalLayer l = noise_temporal_layer(f.ws->d_noise_temporal, a.rows, a.cols, a.channels, k - 1);
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

int rsdsfm_noise_pair_hist_launches(void) { return 1; }

int rsdsfm_noise_curve_resolve_launches(void) { return 1; }

int rsdsfm_denoise_temporal_frame_launches(int32_t rows, int32_t cols, int32_t nsrc, int32_t with_spatial) {
    const int n = rsdsfm_denoise_launches(rows, cols, nsrc);
    return n < 0 ? n
                 : n + (nsrc - 1) * rsdsfm_noise_pair_hist_launches() + rsdsfm_noise_curve_resolve_launches() + (with_spatial ? rsdsfm_denoise_spatial_launches() : 0);
}

int rsdsfm_noise_pair_hist_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image, const uint8_t* d_layer_mask,
                               int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null, int64_t min_overlap, int32_t gain_mode, int32_t first,
                               uint32_t* d_hist8192) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (const char* what = pair_refusal(d_ref_image, d_ref_mask, d_layer_image, d_layer_mask, channels, rows, cols, d_sums8_or_null, min_overlap, gain_mode, first, d_hist8192))
        return stage_fail(c, "noise pair", what);
    return noise_pair_hist_launch(c, d_ref_image, d_ref_mask, d_layer_image, d_layer_mask, channels, rows, cols, reinterpret_cast<const unsigned long long*>(d_sums8_or_null),
                                  min_overlap ? min_overlap : kMinOverlapDefault, gain_mode, first == 1, d_hist8192);
}

int rsdsfm_noise_curve_resolve_dev(rsdsfm_ctx* ctx, const uint32_t* d_hist8192, int32_t quantile_q8, uint64_t* d_curve36_out) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "noise resolve";
    if (quantile_q8 == 0) quantile_q8 = kNoiseQuantileDefault;
    if (quantile_q8 < 1 || quantile_q8 > kNoiseQuantileMax) return stage_fail(c, stage, "quantile_q8 must be in [1, 256] (0: the default, 128)");
    if (!d_hist8192 || !d_curve36_out) return stage_fail(c, stage, "null device pointer");
    if ((uintptr_t)d_hist8192 & 3u) return stage_fail(c, stage, "the histogram must be 4-byte aligned");
    if ((uintptr_t)d_curve36_out & 7u) return stage_fail(c, stage, "the curve must be 8-byte aligned");
    if ((const void*)d_hist8192 == (const void*)d_curve36_out) return stage_fail(c, stage, "the curve may not be the histogram");
    return noise_curve_resolve_launch(c, d_hist8192, quantile_q8, reinterpret_cast<unsigned long long*>(d_curve36_out));
}

int rsdsfm_denoise_temporal_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                                      const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                                      int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_denoise_params* params_or_null,
                                      const rsdsfm_noise_curve_params* curve_or_null, const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null,
                                      uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, uint8_t* d_support_or_null, int64_t* d_counts6_or_null,
                                      uint64_t* d_curve36_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    DeviceGuard device_guard_(&ctx->c);
    return temporal_frame(ctx, EstimatedFrame{d_images, channels, d_depths_colmajor, d_R_rows9, d_t_rows3, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, nsrc, M, m,
                                              params_or_null, spatial_or_null, window_or_null, d_image_out, d_mask_out, d_weight_or_null, d_support_or_null, d_counts6_or_null,
                                              d_curve36_or_null},
                          curve_or_null);
}

int rsdsfm_denoise_temporal_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                                      double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                                      const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                                      const rsdsfm_denoise_params* params_or_null, const rsdsfm_noise_curve_params* curve_or_null,
                                      const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images,
                                      uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null, uint8_t* const* d_out_supports_or_null, int64_t* counts_or_null,
                                      uint64_t* noise_curves_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    DeviceGuard device_guard_(&ctx->c);
    rsdsfm_noise_curve_params np;
    return estimated_clip(ctx, "denoise temporal video",
                          EstimatedClip{d_frames, nsources, rows, cols, channels, fx, fy, cx, cy, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, mode, q5_mode, iterations,
                                        params_or_null, spatial_or_null, window_or_null, d_out_images, d_out_masks, d_out_weights_or_null, d_out_supports_or_null, counts_or_null,
                                        noise_curves_or_null},
                          curve_params_resolve(curve_or_null, &np) ? nullptr : kCurveParamsMessage, kCurveWords,
                          [&](const EstimatedFrame& f) { return temporal_frame(ctx, f, curve_or_null); });
}

}  // extern "C"
