// superres_host.hip -- C ABI of the multi-frame super-resolution (include/rsdsfm_superres.h; tests/superres_spec_numpy.py is the definition,
// superres_kernels.hip the kernels): the render call, the accumulate call, the frame call, which CALLS the public render, record and
// accumulate entry points one after another on planes of the context's dense workspace, and the clip call, which calls the frame call per
// frame, walking the clip as rsdsfm_denoise_video_dev does.
#include "clip_stage_host.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"
#include "stabilize_blend.hpp"
#include "superres.hpp"

namespace rsdsfm {
namespace {

rsdsfm_superres_params superres_defaults() {
    return rsdsfm_superres_params{kSuperresScaleDefault, kSuperresRadiusDefault, kSuperresStrengthDefault, 0, kMinOverlapDefault, (int32_t)sizeof(rsdsfm_superres_params),
                                  {0, 0, 0, 0, 0}};
}

// the params with every 0 of scale, radius, strength and min_overlap replaced by its default, or the defaults for NULL; false: refused
bool superres_params_resolve(const rsdsfm_superres_params* in, rsdsfm_superres_params* out) {
    *out = in ? *in : superres_defaults();
    if (!struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_superres_params))) return false;
    for (int i = 0; i < 5; ++i)
        if (out->reserved[i] != 0) return false;
    if (out->scale == 0) out->scale = kSuperresScaleDefault;
    if (out->radius == 0) out->radius = kSuperresRadiusDefault;
    if (out->strength == 0) out->strength = kSuperresStrengthDefault;
    if (out->min_overlap == 0) out->min_overlap = kMinOverlapDefault;
    return out->scale >= 1 && out->scale <= kSuperresScaleMax && out->radius >= 1 && out->radius <= kSuperresRadiusMax && out->strength >= 1 &&
           out->strength <= kSuperresStrengthMax && out->min_overlap >= 0 && (out->gain_mode == 0 || out->gain_mode == 1);
}

const char* const kSuperresParamsMessage =
    "rsdsfm_superres_params: scale in [1, 4] or 0, radius in [1, 7] or 0, strength in [1, 255] or 0, gain_mode 0 or 1, min_overlap >= 0, reserved 0, struct_bytes 0 or "
    "sizeof (use rsdsfm_superres_params_init)";

// the source size and the scale: the fine size may not pass 16384 either
bool superres_scale_ok(int rows, int cols, int scale) {
    return frame_size_ok(rows, cols, kSuperresSizeMax) && scale >= 1 && scale <= kSuperresScaleMax && (int64_t)scale * rows <= kSuperresSizeMax && (int64_t)scale * cols <= kSuperresSizeMax;
}

const char* const kSuperresScaleMessage = "superres: scale must be in [1, 4] and scale * rows, scale * cols at most 16384";

// the workspace's fine planes, cells and record: made when first asked for and again when the scale changes (a size change releases them with the rest)
int superres_ws(Ctx* c, int rows, int cols, int scale, DenseWs** ws) {
    int rc = rectify_dense_ws(c, rows, cols, ws);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* w = *ws;
    if (w->d_superres && w->superres_scale != scale) {
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // behind whatever the stream still runs on the old planes
        (void)hipFree(w->d_superres);
        w->d_superres = nullptr;
        w->superres_scale = 0;
    }
    if (!w->d_superres) {
        rc = ensure_plane(c, &w->d_superres, superres_ws_bytes(scale * rows, scale * cols), "superres: no memory for the fine planes and the cells");
        if (rc != RSDSFM_OK) return rc;
        w->superres_scale = scale;
    }
    return RSDSFM_OK;
}

static_assert(kSuperresSourcesMax == kClipSourcesMax, "a frame's sources are a ClipPlan's");

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_superres_params_init(rsdsfm_superres_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = superres_defaults();
    return RSDSFM_OK;
}

int rsdsfm_superres_render_launches(int32_t rows, int32_t cols, int32_t scale) {
    if (!superres_scale_ok(rows, cols, scale)) return RSDSFM_ERR_INVALID;
    return rsdsfm_stabilize_window_launches(rows, cols);
}

int rsdsfm_superres_accumulate_launches(void) { return 1; }

int rsdsfm_superres_launches(int32_t rows, int32_t cols, int32_t scale, int32_t nsrc) {
    if (nsrc < 1 || nsrc > kSuperresSourcesMax) return RSDSFM_ERR_INVALID;
    const int one = rsdsfm_superres_render_launches(rows, cols, scale);
    if (one < 0) return one;
    return nsrc * one + (nsrc == 1 ? 1 : (nsrc - 1) * (1 + rsdsfm_superres_accumulate_launches()));
}

int rsdsfm_superres_render_dev(rsdsfm_ctx* ctx, const uint8_t* d_image_n, int32_t channels, const double* d_depth_n_colmajor, const double* d_R_n_rows9,
                               const double* d_t_n_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int mode, int q5_mode,
                               int32_t iterations, const double* M9, const double* m3, int32_t scale, const int32_t* window_or_null, uint8_t* d_bil_out,
                               uint8_t* d_near_out, uint8_t* d_prox_out, uint8_t* d_valid_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (!superres_scale_ok(rows, cols, scale)) return fail(c, RSDSFM_ERR_INVALID, kSuperresScaleMessage);
    if (!d_image_n || !d_depth_n_colmajor || !d_R_n_rows9 || !d_t_n_rows3 || !d_bil_out || !d_near_out || !d_prox_out)
        return fail(c, RSDSFM_ERR_INVALID, "superres render: null device pointer");
    const void* io[5] = {d_image_n, d_bil_out, d_near_out, d_prox_out, d_valid_or_null};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j)
            if (io[j] && io[i] == io[j]) return fail(c, RSDSFM_ERR_INVALID, "superres render: the image and the output planes must be distinct");
    if (((uintptr_t)d_image_n | (uintptr_t)d_bil_out | (uintptr_t)d_near_out | (uintptr_t)d_prox_out | (uintptr_t)d_valid_or_null) & 3u)
        return fail(c, RSDSFM_ERR_INVALID, "superres render: the image and every output plane must be 4-byte aligned");
    if (!M9 || !m3 || !finite_all(M9, 9) || !finite_all(m3, 3))
        return fail(c, RSDSFM_ERR_INVALID, "superres render: the pose (M, m) must be given and finite");
    int32_t full[4];
    const int32_t* window = nullptr;
    rc = frame_window(c, "superres render", window_or_null, rows, cols, full, &window);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    StabPose vp;
    for (int i = 0; i < 9; ++i) vp.M[i] = M9[i];
    for (int i = 0; i < 3; ++i) vp.m[i] = m3[i];
    return superres_render_launch(c, *ws, d_image_n, channels, d_depth_n_colmajor, d_R_n_rows9, d_t_n_rows3, fx, fy, cx, cy, rows, cols, mode, q5_mode,
                                  iterations ? iterations : 3, vp, scale, window, d_bil_out, d_near_out, d_prox_out, d_valid_or_null);
}

int rsdsfm_superres_accumulate_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_bil, const uint8_t* d_ref_near, const uint8_t* d_ref_prox,
                                   const uint8_t* d_layer_bil_or_null, const uint8_t* d_layer_near_or_null, const uint8_t* d_layer_prox_or_null, int32_t channels,
                                   int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null, int64_t min_overlap, int32_t gain_mode, int32_t strength,
                                   uint16_t* d_cells_or_null, int32_t first, int32_t last, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null,
                                   int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if ((first != 0 && first != 1) || (last != 0 && last != 1)) return fail(c, RSDSFM_ERR_INVALID, "superres accumulate: first and last must be 0 or 1");
    if (!frame_size_ok(rows, cols, kSuperresSizeMax)) return fail(c, RSDSFM_ERR_INVALID, "superres: rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "superres: channels must be 1 or 3");
    if (min_overlap < 0 || (gain_mode != 0 && gain_mode != 1) || strength < 0 || strength > kSuperresStrengthMax)
        return fail(c, RSDSFM_ERR_INVALID, "superres accumulate: min_overlap must be >= 0, gain_mode 0 or 1 and strength in [1, 255] (0: the default, 12)");
    if (last) {
        const int rc = output_planes_check(c, "superres", {d_image_out, d_mask_out, d_weight_or_null}, d_counts3_or_null, false);
        if (rc != RSDSFM_OK) return rc;
    } else {  // the outputs are not read
        d_image_out = d_mask_out = d_weight_or_null = nullptr;
        d_counts3_or_null = nullptr;
    }
    if (!d_ref_bil || !d_ref_near || !d_ref_prox) return fail(c, RSDSFM_ERR_INVALID, "superres accumulate: the reference needs its three planes");
    const int nlayer = (d_layer_bil_or_null != nullptr) + (d_layer_near_or_null != nullptr) + (d_layer_prox_or_null != nullptr);
    if (nlayer != 0 && nlayer != 3) return fail(c, RSDSFM_ERR_INVALID, "superres accumulate: the layer needs its three planes, or none");
    if (nlayer == 0 && !(first && last)) return fail(c, RSDSFM_ERR_INVALID, "superres accumulate: without a layer first and last must both be 1");
    if (!d_cells_or_null && !(first && last)) return fail(c, RSDSFM_ERR_INVALID, "superres accumulate: the cells may be NULL only with first and last");
    const void* in[8] = {d_ref_bil, d_ref_near, d_ref_prox, d_layer_bil_or_null, d_layer_near_or_null, d_layer_prox_or_null, d_cells_or_null, d_sums8_or_null};
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            if (in[i] && in[i] == in[j]) return fail(c, RSDSFM_ERR_INVALID, "superres accumulate: the reference's and the layer's planes must be distinct");
    uintptr_t bits = 0;
    for (int i = 0; i < 6; ++i) bits |= (uintptr_t)in[i];
    if (bits & 3u) return fail(c, RSDSFM_ERR_INVALID, "superres: every plane must be 4-byte aligned");
    if (((uintptr_t)d_cells_or_null | (uintptr_t)d_sums8_or_null) & 7u)
        return fail(c, RSDSFM_ERR_INVALID, "superres accumulate: the cells and the record must be 8-byte aligned");
    const void* io[4] = {d_image_out, d_mask_out, d_weight_or_null, d_counts3_or_null};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 8 && io[i]; ++j)
            if (in[j] == io[i]) return fail(c, RSDSFM_ERR_INVALID, "superres accumulate: an output may not be an input, the record or the cells");
    for (int j = 0; j < 6 && d_cells_or_null; ++j)
        if (in[j] == (const void*)d_cells_or_null) return fail(c, RSDSFM_ERR_INVALID, "superres accumulate: the cells may not be an input plane");
    return superres_accumulate_launch(c, d_ref_bil, d_ref_near, d_ref_prox, d_layer_bil_or_null, d_layer_near_or_null, d_layer_prox_or_null, channels, rows, cols,
                                      reinterpret_cast<const unsigned long long*>(d_sums8_or_null), min_overlap ? min_overlap : kMinOverlapDefault, gain_mode,
                                      strength ? strength : kSuperresStrengthDefault, d_cells_or_null, first == 1, last == 1, d_image_out, d_mask_out, d_weight_or_null,
                                      d_counts3_or_null);
}

int rsdsfm_superres_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                              const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                              int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_superres_params* params_or_null,
                              const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc < 1 || nsrc > kSuperresSourcesMax) return fail(c, RSDSFM_ERR_INVALID, "superres frame: nsrc must be in [1, 15]");
    rsdsfm_superres_params sp;
    if (!superres_params_resolve(params_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kSuperresParamsMessage);
    if (!superres_scale_ok(rows, cols, sp.scale)) return fail(c, RSDSFM_ERR_INVALID, kSuperresScaleMessage);
    rc = frame_sources_check(c, "superres frame", d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, nsrc, {d_image_out, d_mask_out, d_weight_or_null});
    if (rc == RSDSFM_OK) rc = frame_poses_check(c, "superres frame", M, m, nsrc);
    if (rc == RSDSFM_OK) rc = output_planes_check(c, "superres", {d_image_out, d_mask_out, d_weight_or_null}, d_counts3_or_null, false);
    int32_t full[4];
    const int32_t* window = nullptr;
    if (rc == RSDSFM_OK) rc = frame_window(c, "superres frame", window_or_null, rows, cols, full, &window);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* ws = nullptr;
    rc = superres_ws(c, rows, cols, sp.scale, &ws);
    if (rc != RSDSFM_OK) return rc;
    const int orows = sp.scale * rows, ocols = sp.scale * cols;
    const size_t P = blend_plane_bytes(orows, ocols);
    uint8_t* b = ws->d_superres;
    uint8_t *rprox = b, *rvalid = b + P, *rbil = b + 2 * P, *rnear = b + 5 * P, *lprox = b + 8 * P, *lbil = b + 9 * P, *lnear = b + 12 * P;
    uint16_t* cells = reinterpret_cast<uint16_t*>(b + 15 * P);
    uint64_t* record = reinterpret_cast<uint64_t*>(b + 23 * P);
    // the public entry points themselves, so that they run the code they run alone
    rc = rsdsfm_superres_render_dev(ctx, d_images[0], channels, d_depths_colmajor[0], d_R_rows9[0], d_t_rows3[0], fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, M, m,
                                    sp.scale, window, rbil, rnear, rprox, rvalid);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc == 1)
        return rsdsfm_superres_accumulate_dev(ctx, rbil, rnear, rprox, nullptr, nullptr, nullptr, channels, orows, ocols, nullptr, sp.min_overlap, sp.gain_mode, sp.strength,
                                              nullptr, 1, 1, d_image_out, d_mask_out, d_weight_or_null, d_counts3_or_null);
    for (int k = 1; k < nsrc; ++k) {
        rc = rsdsfm_superres_render_dev(ctx, d_images[k], channels, d_depths_colmajor[k], d_R_rows9[k], d_t_rows3[k], fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations,
                                        M + 9 * k, m + 3 * k, sp.scale, window, lbil, lnear, lprox, nullptr);
        if (rc != RSDSFM_OK) return rc;
        rc = rsdsfm_seam_overlap_sums_dev(ctx, rbil, rvalid, lbil, lprox, channels, orows, ocols, record);
        if (rc != RSDSFM_OK) return rc;
        rc = rsdsfm_superres_accumulate_dev(ctx, rbil, rnear, rprox, lbil, lnear, lprox, channels, orows, ocols, record, sp.min_overlap, sp.gain_mode, sp.strength, cells,
                                            k == 1, k == nsrc - 1, d_image_out, d_mask_out, d_weight_or_null, d_counts3_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    return RSDSFM_OK;
}

int rsdsfm_superres_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                              double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                              const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                              const rsdsfm_superres_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks,
                              uint8_t* const* d_out_weights_or_null, int64_t* counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    ClipOutputs outs;
    outs.planes[0] = d_out_images;
    outs.planes[1] = d_out_masks;
    outs.planes[2] = d_out_weights_or_null;
    const int rc = clip_arrays_check(c, "superres video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, outs,
                                     "its weight plane when the array is passed");
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_superres_params sp;
    if (!superres_params_resolve(params_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kSuperresParamsMessage);
    // the public entry point itself, so that it runs the code it runs alone
    return walk_clip(c, "superres video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, sp.radius, outs, 3, counts_or_null, [&](const ClipFrame& f) {
        return rsdsfm_superres_frame_dev(ctx, f.img, channels, f.map, f.R, f.t, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, f.plan->nsrc, f.plan->M, f.plan->m,
                                         params_or_null, window_or_null, f.out[0], f.out[1], f.out[2], f.d_counts);
    });
}

}  // extern "C"
