// noise_curve_host.hip -- C ABI of the noise curve (include/rsdsfm_noise_curve.h; tests/noise_curve_spec_numpy.py is the definition,
// noise_curve_kernels.hip the kernels): the primitive, the strength table on the host, the accumulate and the top-up with the strength per pixel
// from a curve, the frame call, which CALLS the public entry points one after another on planes of the context's dense workspace as
// rsdsfm_denoise_auto_frame_dev does, and the clip call, which calls the frame call per frame (walk_clip, clip_stage_host.hpp).
#include <string>
#include <vector>

#include "clip_stage_host.hpp"
#include "denoise.hpp"
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

// every 0 replaced by its default; false: outside its range
bool curve_words_resolve(int32_t* scale, int64_t* min_samples, int64_t* band_min_samples) {
    if (*scale == 0) *scale = kNoiseScaleDefault;
    if (*min_samples == 0) *min_samples = kNoiseMinSamplesDefault;
    if (*band_min_samples == 0) *band_min_samples = kCurveBandMinSamplesDefault;
    return *scale >= 1 && *scale <= kNoiseScaleMax && *min_samples >= 0 && *band_min_samples >= 0;
}

bool curve_quantile_resolve(int32_t* quantile) {
    if (*quantile == 0) *quantile = kNoiseQuantileDefault;
    return *quantile >= 1 && *quantile <= kNoiseQuantileMax;
}

bool curve_params_resolve(const rsdsfm_noise_curve_params* in, rsdsfm_noise_curve_params* out) {
    *out = in ? *in : curve_defaults();
    return struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_noise_curve_params)) && curve_quantile_resolve(&out->quantile_q8) &&
           curve_words_resolve(&out->scale, &out->min_samples, &out->band_min_samples);
}

const char* const kCurveWordsMessage = "scale must be in [1, 255] (0: the default, 12), min_samples >= 0 (0: 1024) and band_min_samples >= 0 (0: 256)";
const char* const kCurveParamsMessage =
    "rsdsfm_noise_curve_params: quantile_q8 in [1, 256] or 0, scale in [1, 255] or 0, min_samples >= 0, band_min_samples >= 0, struct_bytes 0 or sizeof (use "
    "rsdsfm_noise_curve_params_init)";

// what the primitive refuses about its planes, or NULL
const char* curve_planes_refusal(const uint8_t* d_image, const uint8_t* d_mask, int channels, int rows, int cols, const uint32_t* d_hist, const uint64_t* d_curve) {
    if (!frame_size_ok(rows, cols)) return "rows and cols must be in [2, 16384]";
    if (channels != 1 && channels != 3) return "channels must be 1 or 3";
    if (!d_image || !d_mask || !d_hist || !d_curve) return "null device pointer";
    if (((uintptr_t)d_image | (uintptr_t)d_mask | (uintptr_t)d_hist) & 3u) return "the planes and the histogram must be 4-byte aligned";
    if ((uintptr_t)d_curve & 7u) return "the curve must be 8-byte aligned";
    const void *h = d_hist, *r = d_curve;
    if (h == (const void*)d_image || h == (const void*)d_mask || r == (const void*)d_image || r == (const void*)d_mask) return "an output may not be an input";
    if (h == r) return "the outputs must be distinct";
    return nullptr;
}

// a curve the consumers read: given, 8-byte aligned, none of the outputs (NULL entries are skipped)
const char* curve_refusal(const uint64_t* d_curve36, std::initializer_list<const void*> outputs) {
    if (!d_curve36) return "the noise curve is NULL";
    if ((uintptr_t)d_curve36 & 7u) return "the noise curve must be 8-byte aligned";
    for (const void* o : outputs)
        if (o && o == (const void*)d_curve36) return "an output may not be the noise curve";
    return nullptr;
}

int curve_fail(Ctx* c, const char* stage, const char* what) { return fail(c, RSDSFM_ERR_INVALID, (std::string(stage) + ": " + what).c_str()); }

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
    if (!curve_quantile_resolve(&quantile_q8)) return curve_fail(c, "noise curve", "quantile_q8 must be in [1, 256] (0: the default, 128)");
    if (const char* what = curve_planes_refusal(d_image, d_mask, channels, rows, cols, d_hist8192_out, d_curve36_out)) return curve_fail(c, "noise curve", what);
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
        return curve_fail(c, stage, "min_overlap must be >= 0, gain_mode 0 or 1 and strength in [1, 255] (0: the default, 12)");
    if (!curve_words_resolve(&scale, &min_samples, &band_min_samples)) return curve_fail(c, stage, kCurveWordsMessage);
    if (!d_curve36) return curve_fail(c, stage, "the noise curve is NULL");
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
    if (!curve_words_resolve(&scale, &min_samples, &band_min_samples)) return curve_fail(c, stage, kCurveWordsMessage);
    if (const char* what = spatial_planes_refusal(d_image, d_mask, d_weight_or_null, channels, rows, cols, d_image_out, d_support_or_null, d_counts3_or_null))
        return spatial_fail(c, stage, what);
    if (const char* what = curve_refusal(d_curve36, {d_image_out, d_support_or_null, d_counts3_or_null})) return curve_fail(c, stage, what);
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
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "denoise curve frame";
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc < 1 || nsrc > kDenoiseSourcesMax) return curve_fail(c, stage, "nsrc must be in [1, 15]");
    rsdsfm_denoise_params dp;
    if (!denoise_params_resolve(params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDenoiseParamsMessage);
    rsdsfm_noise_curve_params np;
    if (!curve_params_resolve(curve_or_null, &np)) return fail(c, RSDSFM_ERR_INVALID, kCurveParamsMessage);
    const bool top_up = spatial_or_null != nullptr;
    rsdsfm_denoise_spatial_params sp;
    if (!spatial_params_resolve(spatial_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kSpatialParamsMessage);
    if (d_support_or_null && !top_up) return curve_fail(c, stage, "a support plane needs the top-up's parameters");
    rc = frame_sources_check(c, stage, d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, nsrc, {d_image_out, d_mask_out, d_weight_or_null, d_support_or_null});
    if (rc == RSDSFM_OK) rc = frame_poses_check(c, stage, M, m, nsrc);
    if (rc == RSDSFM_OK) rc = output_planes_check(c, stage, {d_image_out, d_mask_out, d_weight_or_null, d_support_or_null}, d_counts6_or_null, true);
    if (rc != RSDSFM_OK) return rc;
    if (d_curve36_or_null) {
        if (const char* what = curve_refusal(d_curve36_or_null, {d_image_out, d_mask_out, d_weight_or_null, d_support_or_null, d_counts6_or_null})) return curve_fail(c, stage, what);
        for (int k = 0; k < nsrc; ++k) {  // the curve is written behind the own render: nothing a later step reads may be it
            const void* const in[4] = {d_images[k], d_depths_colmajor[k], d_R_rows9[k], d_t_rows3[k]};
            for (const void* p : in)
                if (p == (const void*)d_curve36_or_null) return curve_fail(c, stage, "null, misaligned or aliased source pointer");
        }
    }
    int32_t full[4];
    const int32_t* window = nullptr;
    rc = frame_window(c, stage, window_or_null, rows, cols, full, &window);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);  // a size change releases the planes with the rest
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &ws->d_layer, blend_layer_bytes(rows, cols), "denoise curve frame: no memory for the layer");
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &ws->d_denoise, denoise_ws_bytes(rows, cols), "denoise curve frame: no memory for the reference planes and the cells");
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &ws->d_noise_curve, noise_curve_ws_bytes(), "denoise curve frame: no memory for the histogram and the curve");
    if (rc == RSDSFM_OK && top_up)
        rc = ensure_plane(c, &ws->d_denoise_spatial, denoise_spatial_ws_bytes(rows, cols), "denoise curve frame: no memory for the temporal stage's planes");
    if (rc != RSDSFM_OK) return rc;
    const RenderGeom g{channels, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations};
    const DenoisePlanes r = denoise_planes(ws->d_denoise, rows, cols);
    const BlendLayer l = blend_layer(ws->d_layer, rows, cols);
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
    rc = rsdsfm_noise_curve_dev(ctx, r.rimage, r.rmask, channels, rows, cols, np.quantile_q8, nz.hist, d_curve);  // behind the render: the noise the weights compare
    if (rc != RSDSFM_OK) return rc;
    if (nsrc == 1) {
        rc = rsdsfm_denoise_accumulate_curve_dev(ctx, r.rimage, r.rmask, nullptr, nullptr, channels, rows, cols, nullptr, dp.min_overlap, dp.gain_mode, dp.strength, d_curve,
                                                 np.scale, np.min_samples, np.band_min_samples, nullptr, 1, 1, d_image, d_mask_out, d_weight, d_counts6_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    for (int k = 1; k < nsrc; ++k) {
        rc = neighbour_step(ctx, "denoise curve frame: zeroing the layer failed", dp.occlusion == 1, dp.occlusion_tol_q16,
                            source_view(d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, k), g, M + 9 * k, m + 3 * k, window, r.rimage, r.rsource, l.image, l.mask, l.record);
        if (rc != RSDSFM_OK) return rc;
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

int rsdsfm_denoise_curve_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                                   double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                                   const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                                   const rsdsfm_denoise_params* params_or_null, const rsdsfm_noise_curve_params* curve_or_null,
                                   const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images,
                                   uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null, uint8_t* const* d_out_supports_or_null, int64_t* counts_or_null,
                                   uint64_t* noise_curves_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "denoise curve video";
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
    if (!curve_params_resolve(curve_or_null, &np)) return fail(c, RSDSFM_ERR_INVALID, kCurveParamsMessage);
    rsdsfm_denoise_spatial_params sp;
    if (!spatial_params_resolve(spatial_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kSpatialParamsMessage);
    if (d_out_supports_or_null && !spatial_or_null) return curve_fail(c, stage, "the support planes need the top-up's parameters");
    // a frame's 42 device words, [counts: 6][curve: 36], when the caller asks for either: one copy and one wait for both
    constexpr int kWords = 6 + kCurveWords;
    const bool wanted = counts_or_null || noise_curves_or_null;
    std::vector<int64_t> host(wanted ? (size_t)kWords * (size_t)nsources : 0);
    rc = walk_clip(c, stage, d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, dp.radius, outs, kWords, wanted ? host.data() : nullptr,
                   [&](const ClipFrame& f) {
                       return rsdsfm_denoise_curve_frame_dev(ctx, f.img, channels, f.map, f.R, f.t, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, f.plan->nsrc, f.plan->M,
                                                             f.plan->m, params_or_null, curve_or_null, spatial_or_null, window_or_null, f.out[0], f.out[1], f.out[2], f.out[3],
                                                             f.d_counts, f.d_counts ? reinterpret_cast<uint64_t*>(f.d_counts + 6) : nullptr);
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
