// denoise_host.hip -- C ABI of the temporal denoise (include/rsdsfm_denoise.h; tests/denoise_spec_numpy.py is the definition,
// denoise_kernels.hip the kernel): the blend's record as a public call, the accumulate call, the frame call, which CALLS the public render
// entry points, the record call and the accumulate one after another on planes of the context's dense workspace, and the clip call, which
// calls the frame call per frame (walk_clip, clip_stage_host.hpp).
#include "clip_stage_host.hpp"
#include "denoise.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {
namespace {

rsdsfm_denoise_params denoise_defaults() {
    return rsdsfm_denoise_params{RSDSFM_DENOISE_RADIUS_DEFAULT, kDenoiseStrengthDefault, 0, 0, 0, (int32_t)sizeof(rsdsfm_denoise_params), kMinOverlapDefault, {0, 0, 0, 0}};
}

}  // namespace

// the params with every 0 of radius, strength and min_overlap replaced by its default, or the defaults for NULL; false: refused
bool denoise_params_resolve(const rsdsfm_denoise_params* in, rsdsfm_denoise_params* out) {
    *out = in ? *in : denoise_defaults();
    if (!struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_denoise_params))) return false;
    if (out->radius == 0) out->radius = RSDSFM_DENOISE_RADIUS_DEFAULT;
    if (out->strength == 0) out->strength = kDenoiseStrengthDefault;
    if (out->min_overlap == 0) out->min_overlap = kMinOverlapDefault;
    return out->radius >= 1 && out->radius <= kDenoiseRadiusMax && out->strength >= 1 && out->strength <= kDenoiseStrengthMax && out->min_overlap >= 0 &&
           (out->gain_mode == 0 || out->gain_mode == 1) && occlusion_words_ok(out->occlusion, out->occlusion_tol_q16);
}

const char* const kDenoiseParamsMessage =
    "rsdsfm_denoise_params: radius in [1, 7] or 0, strength in [1, 255] or 0, gain_mode 0 or 1, occlusion 0 or 1, occlusion_tol_q16 in [0, 65536], min_overlap >= 0, "
    "struct_bytes 0 or sizeof (use rsdsfm_denoise_params_init)";

namespace {

// the workspace's reference planes and cells, made when first asked for, and the blend's layer
int denoise_ws(Ctx* c, int rows, int cols, DenseWs** ws) {
    int rc = rectify_dense_ws(c, rows, cols, ws);  // a size change releases them with the rest
    if (rc != RSDSFM_OK) return rc;
    rc = ensure_plane(c, &(*ws)->d_layer, blend_layer_bytes(rows, cols), "denoise: no memory for the layer");
    if (rc != RSDSFM_OK) return rc;
    return ensure_plane(c, &(*ws)->d_denoise, denoise_ws_bytes(rows, cols), "denoise: no memory for the reference planes and the cells");
}

static_assert(kDenoiseSourcesMax == kClipSourcesMax, "a frame's sources are a ClipPlan's");

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_denoise_params_init(rsdsfm_denoise_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = denoise_defaults();
    return RSDSFM_OK;
}

int rsdsfm_denoise_accumulate_launches(void) { return 1; }

int rsdsfm_denoise_launches(int32_t rows, int32_t cols, int32_t nsrc) {
    if (nsrc < 1 || nsrc > kDenoiseSourcesMax) return RSDSFM_ERR_INVALID;
    const int one = rsdsfm_stabilize_window_launches(rows, cols);
    if (one < 0) return one;
    return nsrc * one + (nsrc == 1 ? 1 : (nsrc - 1) * (1 + rsdsfm_denoise_accumulate_launches()));
}

int rsdsfm_seam_overlap_sums_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_source, const uint8_t* d_layer, const uint8_t* d_layer_mask,
                                 int32_t channels, int32_t rows, int32_t cols, uint64_t* d_sums8_out) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "seam overlap sums: rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "seam overlap sums: channels must be 1 or 3");
    if (!d_image || !d_source || !d_layer || !d_layer_mask || !d_sums8_out) return fail(c, RSDSFM_ERR_INVALID, "seam overlap sums: null device pointer");
    if (((uintptr_t)d_image | (uintptr_t)d_source | (uintptr_t)d_layer | (uintptr_t)d_layer_mask) & 3u)
        return fail(c, RSDSFM_ERR_INVALID, "seam overlap sums: every plane must be 4-byte aligned");
    if ((uintptr_t)d_sums8_out & 7u) return fail(c, RSDSFM_ERR_INVALID, "seam overlap sums: the record must be 8-byte aligned");
    return seam_overlap_sums_launch(c, d_image, d_source, d_layer, d_layer_mask, channels, rows, cols, reinterpret_cast<unsigned long long*>(d_sums8_out), nullptr);
}

int rsdsfm_denoise_accumulate_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image_or_null,
                                  const uint8_t* d_layer_mask_or_null, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                                  int64_t min_overlap, int32_t gain_mode, int32_t strength, uint16_t* d_cells_or_null, int32_t first, int32_t last,
                                  uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (min_overlap < 0 || (gain_mode != 0 && gain_mode != 1) || strength < 0 || strength > kDenoiseStrengthMax)
        return fail(c, RSDSFM_ERR_INVALID, "denoise accumulate: min_overlap must be >= 0, gain_mode 0 or 1 and strength in [1, 255] (0: the default, 12)");
    AccumulateOutputs out{d_image_out, d_mask_out, d_weight_or_null, d_counts3_or_null};
    const int rc = accumulate_check(c, "denoise", d_ref_image, d_ref_mask, d_layer_image_or_null, d_layer_mask_or_null, channels, rows, cols, d_cells_or_null, {d_sums8_or_null},
                                    first, last, &out);
    if (rc != RSDSFM_OK) return rc;
    return denoise_accumulate_launch(c, d_ref_image, d_ref_mask, d_layer_image_or_null, d_layer_mask_or_null, channels, rows, cols,
                                     reinterpret_cast<const unsigned long long*>(d_sums8_or_null), min_overlap ? min_overlap : kMinOverlapDefault, gain_mode,
                                     strength ? strength : kDenoiseStrengthDefault, d_cells_or_null, first == 1, last == 1, out.image, out.mask, out.weight, out.counts);
}

int rsdsfm_denoise_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                             const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                             int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_denoise_params* params_or_null,
                             const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc < 1 || nsrc > kDenoiseSourcesMax) return fail(c, RSDSFM_ERR_INVALID, "denoise frame: nsrc must be in [1, 15]");
    rsdsfm_denoise_params dp;
    if (!denoise_params_resolve(params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDenoiseParamsMessage);
    rc = frame_sources_check(c, "denoise frame", d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, nsrc, {d_image_out, d_mask_out, d_weight_or_null});
    if (rc == RSDSFM_OK) rc = frame_poses_check(c, "denoise frame", M, m, nsrc);
    if (rc == RSDSFM_OK) rc = output_planes_check(c, "denoise", {d_image_out, d_mask_out, d_weight_or_null}, d_counts3_or_null, false);
    int32_t full[4];
    const int32_t* window = nullptr;
    if (rc == RSDSFM_OK) rc = frame_window(c, "denoise frame", window_or_null, rows, cols, full, &window);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* ws = nullptr;
    rc = denoise_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    const RenderGeom g{channels, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations};
    const DenoisePlanes r = denoise_planes(ws->d_denoise, rows, cols);
    const BlendLayer l = blend_layer(ws->d_layer, rows, cols);
    rc = render_reference(ctx, "denoise frame", source_view(d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, 0), g, M, m, window, r.rimage, r.rmask, r.rsource);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc == 1)
        return rsdsfm_denoise_accumulate_dev(ctx, r.rimage, r.rmask, nullptr, nullptr, channels, rows, cols, nullptr, dp.min_overlap, dp.gain_mode, dp.strength, nullptr, 1, 1,
                                             d_image_out, d_mask_out, d_weight_or_null, d_counts3_or_null);
    for (int k = 1; k < nsrc; ++k) {
        rc = neighbour_step(ctx, "denoise frame: zeroing the layer failed", dp.occlusion == 1, dp.occlusion_tol_q16, source_view(d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, k),
                            g, M + 9 * k, m + 3 * k, window, r.rimage, r.rsource, l.image, l.mask, l.record);
        if (rc != RSDSFM_OK) return rc;
        rc = rsdsfm_denoise_accumulate_dev(ctx, r.rimage, r.rmask, l.image, l.mask, channels, rows, cols, l.record, dp.min_overlap, dp.gain_mode, dp.strength, r.cells, k == 1,
                                           k == nsrc - 1, d_image_out, d_mask_out, d_weight_or_null, d_counts3_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    return RSDSFM_OK;
}

int rsdsfm_denoise_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                             double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                             const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                             const rsdsfm_denoise_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks,
                             uint8_t* const* d_out_weights_or_null, int64_t* counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    ClipOutputs outs;
    outs.planes[0] = d_out_images;
    outs.planes[1] = d_out_masks;
    outs.planes[2] = d_out_weights_or_null;
    const int rc = clip_arrays_check(c, "denoise video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, outs,
                                     "its weight plane when the array is passed");
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_denoise_params dp;
    if (!denoise_params_resolve(params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDenoiseParamsMessage);
    // the public entry point itself, so that it runs the code it runs alone
    return walk_clip(c, "denoise video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, dp.radius, outs, 3, counts_or_null, [&](const ClipFrame& f) {
        return rsdsfm_denoise_frame_dev(ctx, f.img, channels, f.map, f.R, f.t, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, f.plan->nsrc, f.plan->M, f.plan->m,
                                        params_or_null, window_or_null, f.out[0], f.out[1], f.out[2], f.d_counts);
    });
}

}  // extern "C"
