// noise_temporal_host.hip -- C ABI of the temporal noise curve (include/rsdsfm_noise_temporal.h; tests/noise_temporal_spec_numpy.py is the
// definition, noise_temporal_kernels.hip the kernel): the pair histogram, the resolve alone, the frame call, which CALLS the public entry
// points one after another on planes of the context's dense workspace as rsdsfm_denoise_curve_frame_dev does -- with every neighbour kept on
// a stack of layers, because the curve of all of them is resolved before the first accumulate -- and the clip call, which calls the frame call
// per frame (walk_clip, clip_stage_host.hpp).
#include <string>
#include <vector>

#include "clip_stage_host.hpp"
#include "denoise.hpp"
#include "noise_curve.hpp"
#include "noise_temporal.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {
namespace {

int temporal_fail(Ctx* c, const char* stage, const char* what) { return fail(c, RSDSFM_ERR_INVALID, (std::string(stage) + ": " + what).c_str()); }

// the curve's words of a frame call: every 0 replaced by its default; false: outside its range or a wrong struct_bytes (noise_curve_host.hip's rule)
bool temporal_curve_params_resolve(const rsdsfm_noise_curve_params* in, rsdsfm_noise_curve_params* out) {
    if (in)
        *out = *in;
    else
        (void)rsdsfm_noise_curve_params_init(out);
    if (out->quantile_q8 == 0) out->quantile_q8 = kNoiseQuantileDefault;
    if (out->scale == 0) out->scale = kNoiseScaleDefault;
    if (out->min_samples == 0) out->min_samples = kNoiseMinSamplesDefault;
    if (out->band_min_samples == 0) out->band_min_samples = kCurveBandMinSamplesDefault;
    return struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_noise_curve_params)) && out->quantile_q8 >= 1 && out->quantile_q8 <= kNoiseQuantileMax && out->scale >= 1 &&
           out->scale <= kNoiseScaleMax && out->min_samples >= 0 && out->band_min_samples >= 0;
}

const char* const kTemporalCurveParamsMessage =
    "rsdsfm_noise_curve_params: quantile_q8 in [1, 256] or 0, scale in [1, 255] or 0, min_samples >= 0, band_min_samples >= 0, struct_bytes 0 or sizeof (use "
    "rsdsfm_noise_curve_params_init)";

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
        return temporal_fail(c, "noise pair", what);
    return noise_pair_hist_launch(c, d_ref_image, d_ref_mask, d_layer_image, d_layer_mask, channels, rows, cols, reinterpret_cast<const unsigned long long*>(d_sums8_or_null),
                                  min_overlap ? min_overlap : kMinOverlapDefault, gain_mode, first == 1, d_hist8192);
}

int rsdsfm_noise_curve_resolve_dev(rsdsfm_ctx* ctx, const uint32_t* d_hist8192, int32_t quantile_q8, uint64_t* d_curve36_out) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "noise resolve";
    if (quantile_q8 == 0) quantile_q8 = kNoiseQuantileDefault;
    if (quantile_q8 < 1 || quantile_q8 > kNoiseQuantileMax) return temporal_fail(c, stage, "quantile_q8 must be in [1, 256] (0: the default, 128)");
    if (!d_hist8192 || !d_curve36_out) return temporal_fail(c, stage, "null device pointer");
    if ((uintptr_t)d_hist8192 & 3u) return temporal_fail(c, stage, "the histogram must be 4-byte aligned");
    if ((uintptr_t)d_curve36_out & 7u) return temporal_fail(c, stage, "the curve must be 8-byte aligned");
    if ((const void*)d_hist8192 == (const void*)d_curve36_out) return temporal_fail(c, stage, "the curve may not be the histogram");
    return noise_curve_resolve_launch(c, d_hist8192, quantile_q8, reinterpret_cast<unsigned long long*>(d_curve36_out));
}

int rsdsfm_denoise_temporal_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                                      const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                                      int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_denoise_params* params_or_null,
                                      const rsdsfm_noise_curve_params* curve_or_null, const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null,
                                      uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, uint8_t* d_support_or_null, int64_t* d_counts6_or_null,
                                      uint64_t* d_curve36_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "denoise temporal frame";
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc < 1 || nsrc > kDenoiseSourcesMax) return temporal_fail(c, stage, "nsrc must be in [1, 15]");
    rsdsfm_denoise_params dp;
    if (!denoise_params_resolve(params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDenoiseParamsMessage);
    rsdsfm_noise_curve_params np;
    if (!temporal_curve_params_resolve(curve_or_null, &np)) return fail(c, RSDSFM_ERR_INVALID, kTemporalCurveParamsMessage);
    const bool top_up = spatial_or_null != nullptr;
    rsdsfm_denoise_spatial_params sp;
    if (!spatial_params_resolve(spatial_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kSpatialParamsMessage);
    if (d_support_or_null && !top_up) return temporal_fail(c, stage, "a support plane needs the top-up's parameters");
    rc = frame_sources_check(c, stage, d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, nsrc, {d_image_out, d_mask_out, d_weight_or_null, d_support_or_null});
    if (rc == RSDSFM_OK) rc = frame_poses_check(c, stage, M, m, nsrc);
    if (rc == RSDSFM_OK) rc = output_planes_check(c, stage, {d_image_out, d_mask_out, d_weight_or_null, d_support_or_null}, d_counts6_or_null, true);
    if (rc != RSDSFM_OK) return rc;
    if (d_curve36_or_null) {
        if ((uintptr_t)d_curve36_or_null & 7u) return temporal_fail(c, stage, "the noise curve must be 8-byte aligned");
        const void* const outs[5] = {d_image_out, d_mask_out, d_weight_or_null, d_support_or_null, d_counts6_or_null};
        for (const void* o : outs)
            if (o && o == (const void*)d_curve36_or_null) return temporal_fail(c, stage, "an output may not be the noise curve");
        for (int k = 0; k < nsrc; ++k) {  // the curve is written behind the renders: nothing a later step reads may be it
            const void* const in[4] = {d_images[k], d_depths_colmajor[k], d_R_rows9[k], d_t_rows3[k]};
            for (const void* p : in)
                if (p == (const void*)d_curve36_or_null) return temporal_fail(c, stage, "null, misaligned or aliased source pointer");
        }
    }
    int32_t full[4];
    const int32_t* window = nullptr;
    rc = frame_window(c, stage, window_or_null, rows, cols, full, &window);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);  // a size change releases the planes with the rest
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &ws->d_denoise, denoise_ws_bytes(rows, cols), "denoise temporal frame: no memory for the reference planes and the cells");
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &ws->d_noise_curve, noise_curve_ws_bytes(), "denoise temporal frame: no memory for the histogram and the curve");
    if (rc == RSDSFM_OK && nsrc > 1) rc = temporal_stack(c, ws, rows, cols, channels, nsrc - 1);
    if (rc == RSDSFM_OK && top_up)
        rc = ensure_plane(c, &ws->d_denoise_spatial, denoise_spatial_ws_bytes(rows, cols), "denoise temporal frame: no memory for the temporal stage's planes");
    if (rc != RSDSFM_OK) return rc;
    const RenderGeom g{channels, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations};
    const DenoisePlanes r = denoise_planes(ws->d_denoise, rows, cols);
    const NoiseCurvePlanes nz = noise_curve_planes(ws->d_noise_curve);
    uint64_t* const d_curve = d_curve36_or_null ? d_curve36_or_null : nz.curve;
    // the temporal stage's outputs: with the top-up its image (and its weight, when the caller has no plane for it) stay in the workspace
    uint8_t* const d_weight = !top_up || d_weight_or_null ? d_weight_or_null : ws->d_denoise_spatial;
    uint8_t* const d_image = top_up ? ws->d_denoise_spatial + blend_plane_bytes(rows, cols) : d_image_out;
    int64_t* const d_counts3 = d_counts6_or_null ? d_counts6_or_null + 3 : nullptr;
    // what the top-up would refuse, in front of anything enqueued
    if (top_up)
        if (const char* what = spatial_planes_refusal(d_image, d_mask_out, d_weight, channels, rows, cols, d_image_out, d_support_or_null, d_counts3)) return spatial_fail(c, stage, what);

    // the public entry points themselves, so that they run the code they run alone
    rc = render_reference(ctx, stage, source_view(d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, 0), g, M, m, window, r.rimage, r.rmask, r.rsource);
    if (rc != RSDSFM_OK) return rc;
    for (int k = 1; k < nsrc; ++k) {  // every neighbour onto its layer of the stack, its record, its pair histogram
        const NoiseTemporalLayer l = noise_temporal_layer(ws->d_noise_temporal, rows, cols, channels, k - 1);
        rc = neighbour_step(ctx, "denoise temporal frame: zeroing the layer failed", dp.occlusion == 1, dp.occlusion_tol_q16,
                            source_view(d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, k), g, M + 9 * k, m + 3 * k, window, r.rimage, r.rsource, l.image, l.mask, l.record);
        if (rc != RSDSFM_OK) return rc;
        rc = rsdsfm_noise_pair_hist_dev(ctx, r.rimage, r.rmask, l.image, l.mask, channels, rows, cols, l.record, dp.min_overlap, dp.gain_mode, k == 1, nz.hist);
        if (rc != RSDSFM_OK) return rc;
    }
    if (nsrc == 1) RSDSFM_HIP_CHECK(c, hipMemsetAsync(nz.hist, 0, kCurveHistWords * sizeof(uint32_t), c->stream));  // no neighbour: the empty histogram
    rc = rsdsfm_noise_curve_resolve_dev(ctx, nz.hist, np.quantile_q8, d_curve);  // behind every neighbour, in front of the first accumulate
    if (rc != RSDSFM_OK) return rc;
    if (nsrc == 1) {
        rc = rsdsfm_denoise_accumulate_curve_dev(ctx, r.rimage, r.rmask, nullptr, nullptr, channels, rows, cols, nullptr, dp.min_overlap, dp.gain_mode, dp.strength, d_curve,
                                                 np.scale, np.min_samples, np.band_min_samples, nullptr, 1, 1, d_image, d_mask_out, d_weight, d_counts6_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    for (int k = 1; k < nsrc; ++k) {
        const NoiseTemporalLayer l = noise_temporal_layer(ws->d_noise_temporal, rows, cols, channels, k - 1);
        rc = rsdsfm_denoise_accumulate_curve_dev(ctx, r.rimage, r.rmask, l.image, l.mask, channels, rows, cols, l.record, dp.min_overlap, dp.gain_mode, dp.strength, d_curve,
                                                 np.scale, np.min_samples, np.band_min_samples, r.cells, k == 1, k == nsrc - 1, d_image, d_mask_out, d_weight,
                                                 d_counts6_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    if (top_up)
        return rsdsfm_denoise_spatial_curve_dev(ctx, d_image, d_mask_out, d_weight, channels, rows, cols, sp.strength, d_curve, np.scale, np.min_samples, np.band_min_samples,
                                                sp.target, sp.search, d_image_out, d_support_or_null, d_counts3);
    if (d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));  // no top-up: its three counters are 0
    return RSDSFM_OK;
}

int rsdsfm_denoise_temporal_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                                      double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                                      const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                                      const rsdsfm_denoise_params* params_or_null, const rsdsfm_noise_curve_params* curve_or_null,
                                      const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images,
                                      uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null, uint8_t* const* d_out_supports_or_null, int64_t* counts_or_null,
                                      uint64_t* noise_curves_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "denoise temporal video";
    ClipOutputs outs;
    outs.planes[0] = d_out_images;
    outs.planes[1] = d_out_masks;
    outs.planes[2] = d_out_weights_or_null;
    outs.planes[3] = d_out_supports_or_null;
    int rc = clip_arrays_check(c, stage, d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, outs, "its weight and support planes when the arrays are passed");
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_denoise_params dp;  // the radius of the walk is the temporal stage's
    if (!denoise_params_resolve(params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDenoiseParamsMessage);
    rsdsfm_noise_curve_params np;
    if (!temporal_curve_params_resolve(curve_or_null, &np)) return fail(c, RSDSFM_ERR_INVALID, kTemporalCurveParamsMessage);
    rsdsfm_denoise_spatial_params sp;
    if (!spatial_params_resolve(spatial_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kSpatialParamsMessage);
    if (d_out_supports_or_null && !spatial_or_null) return temporal_fail(c, stage, "the support planes need the top-up's parameters");
    // a frame's 42 device words, [counts: 6][curve: 36], when the caller asks for either: one copy and one wait for both
    constexpr int kWords = 6 + kCurveWords;
    const bool wanted = counts_or_null || noise_curves_or_null;
    std::vector<int64_t> host(wanted ? (size_t)kWords * (size_t)nsources : 0);
    rc = walk_clip(c, stage, d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, dp.radius, outs, kWords, wanted ? host.data() : nullptr,
                   [&](const ClipFrame& f) {
                       return rsdsfm_denoise_temporal_frame_dev(ctx, f.img, channels, f.map, f.R, f.t, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, f.plan->nsrc,
                                                                f.plan->M, f.plan->m, params_or_null, curve_or_null, spatial_or_null, window_or_null, f.out[0], f.out[1], f.out[2],
                                                                f.out[3], f.d_counts, f.d_counts ? reinterpret_cast<uint64_t*>(f.d_counts + 6) : nullptr);
                   });
    if (rc != RSDSFM_OK || !wanted) return rc;
    for (int q = 0; q < nsources; ++q) {
        const int64_t* w = host.data() + (size_t)kWords * (size_t)q;
        for (int k = 0; k < 6 && counts_or_null; ++k) counts_or_null[6 * (size_t)q + k] = w[k];
        for (int k = 0; k < kCurveWords && noise_curves_or_null; ++k) noise_curves_or_null[(size_t)kCurveWords * (size_t)q + k] = (uint64_t)w[6 + k];
    }
    return RSDSFM_OK;
}

}  // extern "C"
