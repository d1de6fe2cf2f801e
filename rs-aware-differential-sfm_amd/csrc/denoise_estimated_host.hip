// denoise_estimated_host.hip -- denoise_estimated_host.hpp's out-of-line part: the front and the tail of a frame call and the clip call of the
// estimated-strength denoise, and the refusals its stages share.  (The clip call is a template in the header, as walk_clip is.)
#include "denoise_estimated_host.hpp"

#include <string>

namespace rsdsfm {

int stage_fail(Ctx* c, const char* stage, const char* what) { return fail(c, RSDSFM_ERR_INVALID, (std::string(stage) + ": " + what).c_str()); }

// the texts, for a search: "the noise record is NULL", "the noise curve is NULL", "the noise record must be 8-byte aligned", "the noise curve must be
// 8-byte aligned", "an output may not be the noise record", "an output may not be the noise curve"
int estimate_check(Ctx* c, const char* stage, const char* noun, const uint64_t* d_estimate, std::initializer_list<const void*> outputs) {
    const std::string the = std::string("the ") + noun;
    if (!d_estimate) return stage_fail(c, stage, (the + " is NULL").c_str());
    if ((uintptr_t)d_estimate & 7u) return stage_fail(c, stage, (the + " must be 8-byte aligned").c_str());
    for (const void* o : outputs)
        if (o && o == (const void*)d_estimate) return stage_fail(c, stage, ("an output may not be " + the).c_str());
    return RSDSFM_OK;
}

// the assembled texts, for a search: "the record must be 8-byte aligned", "the curve must be 8-byte aligned"
int measure_planes_check(Ctx* c, const char* stage, const char* noun, const uint8_t* d_image, const uint8_t* d_mask, int channels, int rows, int cols, const uint32_t* d_hist,
                         const uint64_t* d_estimate) {
    if (!frame_size_ok(rows, cols)) return stage_fail(c, stage, "rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return stage_fail(c, stage, "channels must be 1 or 3");
    if (!d_image || !d_mask || !d_hist || !d_estimate) return stage_fail(c, stage, "null device pointer");
    if (((uintptr_t)d_image | (uintptr_t)d_mask | (uintptr_t)d_hist) & 3u) return stage_fail(c, stage, "the planes and the histogram must be 4-byte aligned");
    if ((uintptr_t)d_estimate & 7u) return stage_fail(c, stage, (std::string("the ") + noun + " must be 8-byte aligned").c_str());
    const void *h = d_hist, *r = d_estimate;
    if (h == (const void*)d_image || h == (const void*)d_mask || r == (const void*)d_image || r == (const void*)d_mask) return stage_fail(c, stage, "an output may not be an input");
    if (h == r) return stage_fail(c, stage, "the outputs must be distinct");
    return RSDSFM_OK;
}

int estimated_checks(rsdsfm_ctx* ctx, const char* stage, const char* noun, const EstimatedFrame& a, const char* estimator_refusal, EstimatedFront* front) {
    Ctx* c = &ctx->c;
    EstimatedFront& f = *front;
    int rc = rectify_dense_check(c, a.channels, a.rows, a.cols, a.mode, a.q5_mode, a.iterations);
    if (rc != RSDSFM_OK) return rc;
    if (a.nsrc < 1 || a.nsrc > kDenoiseSourcesMax) return stage_fail(c, stage, "nsrc must be in [1, 15]");
    if (!denoise_params_resolve(a.params_or_null, &f.dp)) return fail(c, RSDSFM_ERR_INVALID, kDenoiseParamsMessage);
    if (estimator_refusal) return fail(c, RSDSFM_ERR_INVALID, estimator_refusal);
    f.top_up = a.spatial_or_null != nullptr;
    if (!spatial_params_resolve(a.spatial_or_null, &f.sp)) return fail(c, RSDSFM_ERR_INVALID, kSpatialParamsMessage);
    if (a.d_support_or_null && !f.top_up) return stage_fail(c, stage, "a support plane needs the top-up's parameters");
    rc = frame_sources_check(c, stage, a.d_images, a.d_depths_colmajor, a.d_R_rows9, a.d_t_rows3, a.nsrc, {a.d_image_out, a.d_mask_out, a.d_weight_or_null, a.d_support_or_null});
    if (rc == RSDSFM_OK) rc = frame_poses_check(c, stage, a.M, a.m, a.nsrc);
    if (rc == RSDSFM_OK) rc = output_planes_check(c, stage, {a.d_image_out, a.d_mask_out, a.d_weight_or_null, a.d_support_or_null}, a.d_counts6_or_null, true);
    if (rc != RSDSFM_OK) return rc;
    if (a.d_estimate_or_null) {
        rc = estimate_check(c, stage, noun, a.d_estimate_or_null, {a.d_image_out, a.d_mask_out, a.d_weight_or_null, a.d_support_or_null, a.d_counts6_or_null});
        if (rc != RSDSFM_OK) return rc;
        for (int k = 0; k < a.nsrc; ++k) {  // the estimate is written behind the own render: nothing a later step reads may be it
            const void* const in[4] = {a.d_images[k], a.d_depths_colmajor[k], a.d_R_rows9[k], a.d_t_rows3[k]};
            for (const void* p : in)
                if (p == (const void*)a.d_estimate_or_null) return stage_fail(c, stage, "null, misaligned or aliased source pointer");
        }
    }
    rc = frame_window(c, stage, a.window_or_null, a.rows, a.cols, f.full, &f.window);
    if (rc != RSDSFM_OK) return rc;
    return rectify_dense_ws(c, a.rows, a.cols, &f.ws);  // a size change releases the planes with the rest
}

int estimated_render(rsdsfm_ctx* ctx, const char* stage, const EstimatedFrame& a, uint64_t* d_estimate_ws, EstimatedFront* front) {
    Ctx* c = &ctx->c;
    EstimatedFront& f = *front;
    int rc = RSDSFM_OK;
    if (f.top_up)
        rc = ensure_plane(c, &f.ws->d_denoise_spatial, denoise_spatial_ws_bytes(a.rows, a.cols), (std::string(stage) + ": no memory for the temporal stage's planes").c_str());
    if (rc != RSDSFM_OK) return rc;
    f.g = RenderGeom{a.channels, a.fx, a.fy, a.cx, a.cy, a.rows, a.cols, a.mode, a.q5_mode, a.iterations};
    f.r = denoise_planes(f.ws->d_denoise, a.rows, a.cols);
    f.d_estimate = a.d_estimate_or_null ? a.d_estimate_or_null : d_estimate_ws;
    f.d_weight = !f.top_up || a.d_weight_or_null ? a.d_weight_or_null : f.ws->d_denoise_spatial;
    f.d_image = f.top_up ? f.ws->d_denoise_spatial + blend_plane_bytes(a.rows, a.cols) : a.d_image_out;
    f.d_counts3 = a.d_counts6_or_null ? a.d_counts6_or_null + 3 : nullptr;
    // what the top-up would refuse, in front of anything enqueued
    if (f.top_up)
        if (const char* what = spatial_planes_refusal(f.d_image, a.d_mask_out, f.d_weight, a.channels, a.rows, a.cols, a.d_image_out, a.d_support_or_null, f.d_counts3))
            return spatial_fail(c, stage, what);
    // the public entry points themselves, so that they run the code they run alone
    return render_reference(ctx, stage, source_view(a.d_images, a.d_depths_colmajor, a.d_R_rows9, a.d_t_rows3, 0), f.g, a.M, a.m, f.window, f.r.rimage, f.r.rmask, f.r.rsource);
}

int estimated_tail(Ctx* c, const EstimatedFront& front) {
    if (front.d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(front.d_counts3, 0, 3 * sizeof(int64_t), c->stream));  // no top-up: its three counters are 0
    return RSDSFM_OK;
}

}  // namespace rsdsfm
