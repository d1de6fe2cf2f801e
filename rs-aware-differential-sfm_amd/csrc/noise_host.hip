// noise_host.hip -- C ABI of the noise level (include/rsdsfm_noise.h; tests/noise_spec_numpy.py is the definition, noise_kernels.hip the
// kernels): the primitive, the strength on the host, the accumulate and the top-up with the strength from a record, the frame call, which
// CALLS the public entry points one after another on planes of the context's dense workspace as rsdsfm_denoise_frame_dev does, and the clip
// call, which calls the frame call per frame (walk_clip, clip_stage_host.hpp).
#include <string>
#include <vector>

#include "clip_stage_host.hpp"
#include "denoise.hpp"
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

// what the primitive refuses about its planes, or NULL
const char* noise_planes_refusal(const uint8_t* d_image, const uint8_t* d_mask, int channels, int rows, int cols, const uint32_t* d_hist, const uint64_t* d_record) {
    if (!frame_size_ok(rows, cols)) return "rows and cols must be in [2, 16384]";
    if (channels != 1 && channels != 3) return "channels must be 1 or 3";
    if (!d_image || !d_mask || !d_hist || !d_record) return "null device pointer";
    if (((uintptr_t)d_image | (uintptr_t)d_mask | (uintptr_t)d_hist) & 3u) return "the planes and the histogram must be 4-byte aligned";
    if ((uintptr_t)d_record & 7u) return "the record must be 8-byte aligned";
    const void *h = d_hist, *r = d_record;
    if (h == (const void*)d_image || h == (const void*)d_mask || r == (const void*)d_image || r == (const void*)d_mask) return "an output may not be an input";
    if (h == r) return "the outputs must be distinct";
    return nullptr;
}

// a record the auto calls read: given, 8-byte aligned, none of the outputs (NULL entries are skipped)
const char* record_refusal(const uint64_t* d_noise4, std::initializer_list<const void*> outputs) {
    if (!d_noise4) return "the noise record is NULL";
    if ((uintptr_t)d_noise4 & 7u) return "the noise record must be 8-byte aligned";
    for (const void* o : outputs)
        if (o && o == (const void*)d_noise4) return "an output may not be the noise record";
    return nullptr;
}

int noise_fail(Ctx* c, const char* stage, const char* what) { return fail(c, RSDSFM_ERR_INVALID, (std::string(stage) + ": " + what).c_str()); }

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
    if (!quantile_resolve(&quantile_q8)) return noise_fail(c, "noise level", "quantile_q8 must be in [1, 256] (0: the default, 128)");
    if (const char* what = noise_planes_refusal(d_image, d_mask, channels, rows, cols, d_hist1024_out, d_record4_out)) return noise_fail(c, "noise level", what);
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
        return noise_fail(c, stage, "min_overlap must be >= 0, gain_mode 0 or 1 and strength in [1, 255] (0: the default, 12)");
    if (!noise_words_resolve(&scale, &min_samples)) return noise_fail(c, stage, kNoiseWordsMessage);
    if (!d_noise4) return noise_fail(c, stage, "the noise record is NULL");
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
    if (!noise_words_resolve(&scale, &min_samples)) return noise_fail(c, stage, kNoiseWordsMessage);
    if (const char* what = spatial_planes_refusal(d_image, d_mask, d_weight_or_null, channels, rows, cols, d_image_out, d_support_or_null, d_counts3_or_null))
        return spatial_fail(c, stage, what);
    if (const char* what = record_refusal(d_noise4, {d_image_out, d_support_or_null, d_counts3_or_null})) return noise_fail(c, stage, what);
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
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "denoise auto frame";
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc < 1 || nsrc > kDenoiseSourcesMax) return noise_fail(c, stage, "nsrc must be in [1, 15]");
    rsdsfm_denoise_params dp;
    if (!denoise_params_resolve(params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDenoiseParamsMessage);
    rsdsfm_noise_params np;
    if (!noise_params_resolve(noise_or_null, &np)) return fail(c, RSDSFM_ERR_INVALID, kNoiseParamsMessage);
    const bool top_up = spatial_or_null != nullptr;
    rsdsfm_denoise_spatial_params sp;
    if (!spatial_params_resolve(spatial_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kSpatialParamsMessage);
    if (d_support_or_null && !top_up) return noise_fail(c, stage, "a support plane needs the top-up's parameters");
    rc = frame_sources_check(c, stage, d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, nsrc, {d_image_out, d_mask_out, d_weight_or_null, d_support_or_null});
    if (rc == RSDSFM_OK) rc = frame_poses_check(c, stage, M, m, nsrc);
    if (rc == RSDSFM_OK) rc = output_planes_check(c, stage, {d_image_out, d_mask_out, d_weight_or_null, d_support_or_null}, d_counts6_or_null, true);
    if (rc != RSDSFM_OK) return rc;
    if (d_noise4_or_null) {
        if (const char* what = record_refusal(d_noise4_or_null, {d_image_out, d_mask_out, d_weight_or_null, d_support_or_null, d_counts6_or_null})) return noise_fail(c, stage, what);
        for (int k = 0; k < nsrc; ++k) {  // the record is written behind the own render: nothing a later step reads may be it
            const void* const in[4] = {d_images[k], d_depths_colmajor[k], d_R_rows9[k], d_t_rows3[k]};
            for (const void* p : in)
                if (p == (const void*)d_noise4_or_null) return noise_fail(c, stage, "null, misaligned or aliased source pointer");
        }
    }
    int32_t full[4];
    const int32_t* window = nullptr;
    rc = frame_window(c, stage, window_or_null, rows, cols, full, &window);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);  // a size change releases the planes with the rest
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &ws->d_layer, blend_layer_bytes(rows, cols), "denoise auto frame: no memory for the layer");
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &ws->d_denoise, denoise_ws_bytes(rows, cols), "denoise auto frame: no memory for the reference planes and the cells");
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &ws->d_noise, noise_ws_bytes(), "denoise auto frame: no memory for the histogram and the record");
    if (rc == RSDSFM_OK && top_up)
        rc = ensure_plane(c, &ws->d_denoise_spatial, denoise_spatial_ws_bytes(rows, cols), "denoise auto frame: no memory for the temporal stage's planes");
    if (rc != RSDSFM_OK) return rc;
    const RenderGeom g{channels, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations};
    const DenoisePlanes r = denoise_planes(ws->d_denoise, rows, cols);
    const BlendLayer l = blend_layer(ws->d_layer, rows, cols);
    const NoisePlanes nz = noise_planes(ws->d_noise);
    uint64_t* const d_record = d_noise4_or_null ? d_noise4_or_null : nz.record;
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
    rc = rsdsfm_noise_level_dev(ctx, r.rimage, r.rmask, channels, rows, cols, np.quantile_q8, nz.hist, d_record);  // behind the render: the noise the weights compare
    if (rc != RSDSFM_OK) return rc;
    if (nsrc == 1) {
        rc = rsdsfm_denoise_accumulate_auto_dev(ctx, r.rimage, r.rmask, nullptr, nullptr, channels, rows, cols, nullptr, dp.min_overlap, dp.gain_mode, dp.strength, d_record,
                                                np.scale, np.min_samples, nullptr, 1, 1, d_image, d_mask_out, d_weight, d_counts6_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    for (int k = 1; k < nsrc; ++k) {
        rc = neighbour_step(ctx, "denoise auto frame: zeroing the layer failed", dp.occlusion == 1, dp.occlusion_tol_q16,
                            source_view(d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, k), g, M + 9 * k, m + 3 * k, window, r.rimage, r.rsource, l.image, l.mask, l.record);
        if (rc != RSDSFM_OK) return rc;
        rc = rsdsfm_denoise_accumulate_auto_dev(ctx, r.rimage, r.rmask, l.image, l.mask, channels, rows, cols, l.record, dp.min_overlap, dp.gain_mode, dp.strength, d_record,
                                                np.scale, np.min_samples, r.cells, k == 1, k == nsrc - 1, d_image, d_mask_out, d_weight, d_counts6_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    if (top_up)
        return rsdsfm_denoise_spatial_auto_dev(ctx, d_image, d_mask_out, d_weight, channels, rows, cols, sp.strength, d_record, np.scale, np.min_samples, sp.target, sp.search,
                                               d_image_out, d_support_or_null, d_counts3);
    if (d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));  // no top-up: its three counters are 0
    return RSDSFM_OK;
}

int rsdsfm_denoise_auto_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                                  double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                                  const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                                  const rsdsfm_denoise_params* params_or_null, const rsdsfm_noise_params* noise_or_null,
                                  const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images,
                                  uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null, uint8_t* const* d_out_supports_or_null, int64_t* counts_or_null,
                                  uint64_t* noise_records_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "denoise auto video";
    ClipOutputs outs;
    outs.planes[0] = d_out_images;
    outs.planes[1] = d_out_masks;
    outs.planes[2] = d_out_weights_or_null;
    outs.planes[3] = d_out_supports_or_null;
    int rc = clip_arrays_check(c, stage, d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, outs, "its weight and support planes when the arrays are passed");
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_denoise_params dp;  // the radius of the walk is the temporal stage's
    if (!denoise_params_resolve(params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDenoiseParamsMessage);
    rsdsfm_noise_params np;
    if (!noise_params_resolve(noise_or_null, &np)) return fail(c, RSDSFM_ERR_INVALID, kNoiseParamsMessage);
    rsdsfm_denoise_spatial_params sp;
    if (!spatial_params_resolve(spatial_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kSpatialParamsMessage);
    if (d_out_supports_or_null && !spatial_or_null) return noise_fail(c, stage, "the support planes need the top-up's parameters");
    // a frame's ten device words, [counts: 6][record: 4], when the caller asks for either: one copy and one wait for both
    constexpr int kWords = 10;
    const bool wanted = counts_or_null || noise_records_or_null;
    std::vector<int64_t> host(wanted ? (size_t)kWords * (size_t)nsources : 0);
    rc = walk_clip(c, stage, d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, dp.radius, outs, kWords, wanted ? host.data() : nullptr,
                   [&](const ClipFrame& f) {
                       return rsdsfm_denoise_auto_frame_dev(ctx, f.img, channels, f.map, f.R, f.t, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, f.plan->nsrc, f.plan->M,
                                                            f.plan->m, params_or_null, noise_or_null, spatial_or_null, window_or_null, f.out[0], f.out[1], f.out[2], f.out[3],
                                                            f.d_counts, f.d_counts ? reinterpret_cast<uint64_t*>(f.d_counts + 6) : nullptr);
                   });
    if (rc != RSDSFM_OK || !wanted) return rc;
    for (int q = 0; q < nsources; ++q) {
        const int64_t* w = host.data() + (size_t)kWords * (size_t)q;
        for (int k = 0; k < 6 && counts_or_null; ++k) counts_or_null[6 * (size_t)q + k] = w[k];
        for (int k = 0; k < 4 && noise_records_or_null; ++k) noise_records_or_null[4 * (size_t)q + k] = (uint64_t)w[6 + k];
    }
    return RSDSFM_OK;
}

}  // extern "C"
