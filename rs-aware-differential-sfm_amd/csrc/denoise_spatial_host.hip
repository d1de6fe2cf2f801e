// denoise_spatial_host.hip -- C ABI of the spatial top-up (include/rsdsfm_denoise_spatial.h; tests/denoise_spatial_spec_numpy.py is the definition,
// denoise_spatial_kernels.hip the kernel): the primitive, the frame call, which CALLS the public temporal frame call into planes of the context's
// dense workspace and the primitive behind it, and the clip call, which calls the frame call per frame (walk_clip, clip_stage_host.hpp).
#include <string>

#include "clip_stage_host.hpp"
#include "denoise.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {
namespace {

rsdsfm_denoise_spatial_params spatial_defaults() {
    return rsdsfm_denoise_spatial_params{kDenoiseStrengthDefault, kDenoiseSpatialTargetDefault, kDenoiseSpatialSearchDefault, (int32_t)sizeof(rsdsfm_denoise_spatial_params),
                                         {0, 0, 0, 0}};
}

}  // namespace

// every 0 replaced by its default; false: outside its range (declared in denoise.hpp: the auto calls of noise_host.hip refuse in the same words)
bool spatial_words_resolve(int32_t* strength, int32_t* target, int32_t* search) {
    if (*strength == 0) *strength = kDenoiseStrengthDefault;
    if (*target == 0) *target = kDenoiseSpatialTargetDefault;
    if (*search == 0) *search = kDenoiseSpatialSearchDefault;
    return *strength >= 1 && *strength <= kDenoiseStrengthMax && *target >= 1 && *target <= kDenoiseSpatialTargetMax && *search >= 1 && *search <= kDenoiseSpatialSearchMax;
}

bool spatial_params_resolve(const rsdsfm_denoise_spatial_params* in, rsdsfm_denoise_spatial_params* out) {
    *out = in ? *in : spatial_defaults();
    return struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_denoise_spatial_params)) && spatial_words_resolve(&out->strength, &out->target, &out->search);
}

const char* const kSpatialWordsMessage = "strength must be in [1, 255] (0: the default, 12), target in [1, 255] (0: 80) and search in [1, 3] (0: 2)";
const char* const kSpatialParamsMessage =
    "rsdsfm_denoise_spatial_params: strength in [1, 255] or 0, target in [1, 255] or 0, search in [1, 3] or 0, struct_bytes 0 or sizeof (use "
    "rsdsfm_denoise_spatial_params_init)";

// what the primitive refuses about its planes, or NULL
const char* spatial_planes_refusal(const uint8_t* d_image, const uint8_t* d_mask, const uint8_t* d_weight, int channels, int rows, int cols, const uint8_t* d_image_out,
                                   const uint8_t* d_support, const int64_t* d_counts3) {
    if (!frame_size_ok(rows, cols)) return "rows and cols must be in [2, 16384]";
    if (channels != 1 && channels != 3) return "channels must be 1 or 3";
    if (!d_image || !d_mask || !d_image_out) return "null device pointer";
    if (((uintptr_t)d_image | (uintptr_t)d_mask | (uintptr_t)d_weight | (uintptr_t)d_image_out | (uintptr_t)d_support) & 3u) return "every plane must be 4-byte aligned";
    if ((uintptr_t)d_counts3 & 7u) return "the counters must be 8-byte aligned";
    const void* in[3] = {d_image, d_mask, d_weight};
    const void* io[3] = {d_image_out, d_support, d_counts3};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3 && io[i]; ++j)
            if (io[i] == in[j]) return "an output may not be an input";
        for (int j = i + 1; j < 3 && io[i]; ++j)
            if (io[i] == io[j]) return "the outputs must be distinct";
    }
    return nullptr;
}

int spatial_fail(Ctx* c, const char* stage, const char* what) { return fail(c, RSDSFM_ERR_INVALID, (std::string(stage) + ": " + what).c_str()); }

}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_denoise_spatial_params_init(rsdsfm_denoise_spatial_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = spatial_defaults();
    return RSDSFM_OK;
}

int rsdsfm_denoise_spatial_launches(void) { return 1; }

int rsdsfm_denoise_spatial_frame_launches(int32_t rows, int32_t cols, int32_t nsrc) {
    const int n = rsdsfm_denoise_launches(rows, cols, nsrc);
    return n < 0 ? n : n + rsdsfm_denoise_spatial_launches();
}

int rsdsfm_denoise_spatial_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, const uint8_t* d_weight_or_null, int32_t channels, int32_t rows,
                               int32_t cols, int32_t strength, int32_t target, int32_t search, uint8_t* d_image_out, uint8_t* d_support_or_null,
                               int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!spatial_words_resolve(&strength, &target, &search)) return spatial_fail(c, "denoise spatial", kSpatialWordsMessage);
    if (const char* what = spatial_planes_refusal(d_image, d_mask, d_weight_or_null, channels, rows, cols, d_image_out, d_support_or_null, d_counts3_or_null))
        return spatial_fail(c, "denoise spatial", what);
    return denoise_spatial_launch(c, d_image, d_mask, d_weight_or_null, channels, rows, cols, strength, target, search, d_image_out, d_support_or_null, d_counts3_or_null);
}

int rsdsfm_denoise_spatial_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                                     const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows,
                                     int32_t cols, int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m,
                                     const rsdsfm_denoise_params* params_or_null, const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null,
                                     uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, uint8_t* d_support_or_null, int64_t* d_counts6_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const char* const stage = "denoise spatial frame";
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc < 1 || nsrc > kDenoiseSourcesMax) return spatial_fail(c, stage, "nsrc must be in [1, 15]");
    rsdsfm_denoise_params dp;
    if (!denoise_params_resolve(params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDenoiseParamsMessage);
    rsdsfm_denoise_spatial_params sp;
    if (!spatial_params_resolve(spatial_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kSpatialParamsMessage);
    rc = frame_sources_check(c, stage, d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, nsrc, {d_image_out, d_mask_out, d_weight_or_null, d_support_or_null});
    if (rc == RSDSFM_OK) rc = frame_poses_check(c, stage, M, m, nsrc);
    if (rc == RSDSFM_OK) rc = output_planes_check(c, stage, {d_image_out, d_mask_out, d_weight_or_null, d_support_or_null}, d_counts6_or_null, true);
    int32_t full[4];
    const int32_t* window = nullptr;
    if (rc == RSDSFM_OK) rc = frame_window(c, stage, window_or_null, rows, cols, full, &window);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);  // a size change releases the plane with the rest
    if (rc == RSDSFM_OK) rc = ensure_plane(c, &ws->d_denoise_spatial, denoise_spatial_ws_bytes(rows, cols), "denoise spatial frame: no memory for the temporal stage's planes");
    if (rc != RSDSFM_OK) return rc;
    uint8_t* const d_weight = d_weight_or_null ? d_weight_or_null : ws->d_denoise_spatial;
    uint8_t* const d_image = ws->d_denoise_spatial + blend_plane_bytes(rows, cols);
    int64_t* const d_counts3 = d_counts6_or_null ? d_counts6_or_null + 3 : nullptr;
    // what the primitive would refuse, in front of anything enqueued
    if (const char* what = spatial_planes_refusal(d_image, d_mask_out, d_weight, channels, rows, cols, d_image_out, d_support_or_null, d_counts3)) return spatial_fail(c, stage, what);
    // the public entry points themselves, so that they run the code they run alone
    rc = rsdsfm_denoise_frame_dev(ctx, d_images, channels, d_depths_colmajor, d_R_rows9, d_t_rows3, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, nsrc, M, m, params_or_null,
                                  window_or_null, d_image, d_mask_out, d_weight, d_counts6_or_null);
    if (rc != RSDSFM_OK) return rc;
    return rsdsfm_denoise_spatial_dev(ctx, d_image, d_mask_out, d_weight, channels, rows, cols, sp.strength, sp.target, sp.search, d_image_out, d_support_or_null, d_counts3);
}

int rsdsfm_denoise_spatial_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx,
                                     double fy, double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t,
                                     const double* A, const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode,
                                     int32_t iterations, const rsdsfm_denoise_params* params_or_null, const rsdsfm_denoise_spatial_params* spatial_or_null,
                                     const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null,
                                     uint8_t* const* d_out_supports_or_null, int64_t* counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    ClipOutputs outs;
    outs.planes[0] = d_out_images;
    outs.planes[1] = d_out_masks;
    outs.planes[2] = d_out_weights_or_null;
    outs.planes[3] = d_out_supports_or_null;
    const int rc = clip_arrays_check(c, "denoise spatial video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, outs,
                                     "its weight and support planes when the arrays are passed");
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_denoise_params dp;  // the radius of the walk is the temporal stage's
    if (!denoise_params_resolve(params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDenoiseParamsMessage);
    rsdsfm_denoise_spatial_params sp;
    if (!spatial_params_resolve(spatial_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kSpatialParamsMessage);
    return walk_clip(c, "denoise spatial video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, dp.radius, outs, 6, counts_or_null,
                     [&](const ClipFrame& f) {
                         return rsdsfm_denoise_spatial_frame_dev(ctx, f.img, channels, f.map, f.R, f.t, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, f.plan->nsrc,
                                                                 f.plan->M, f.plan->m, params_or_null, spatial_or_null, window_or_null, f.out[0], f.out[1], f.out[2], f.out[3],
                                                                 f.d_counts);
                     });
}

}  // extern "C"
