// stabilize_inpaint_host.hip -- C ABI of the stabiliser's inpainting (include/rsdsfm_stabilize_inpaint.h; tests/stabilize_inpaint_spec_numpy.py
// is the definition, stabilize_inpaint_kernels.hip the kernels): the frame call, which only enqueues, its launch count, and the clip call,
// which CALLS the public entry points one after another.
#include "../../include/rsdsfm_stabilize_inpaint.h"
#include "clip_stage_host.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "last_frame.hpp"
#include "sequence_host.hpp"
#include "stabilize_inpaint.hpp"

namespace rsdsfm {
namespace {

static_assert(RSDSFM_SOURCE_INPAINTED == kSourceInpainted, "the header's id is the kernels'");

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_inpaint_launches(int32_t rows, int32_t cols) { return frame_size_ok(rows, cols) ? inpaint_launch_count(rows, cols) : RSDSFM_ERR_INVALID; }

int rsdsfm_inpaint_frame_dev(rsdsfm_ctx* ctx, uint8_t* d_image_inout, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols,
                             uint8_t* d_source_or_null, int64_t* d_count_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "inpaint: rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "inpaint: channels must be 1 or 3");
    if (!d_image_inout || !d_mask) return fail(c, RSDSFM_ERR_INVALID, "inpaint: null device pointer (the image and the mask are required)");
    if (d_image_inout == d_mask || (d_source_or_null && (d_source_or_null == d_mask || d_source_or_null == d_image_inout)))
        return fail(c, RSDSFM_ERR_INVALID, "inpaint: the image, the mask and the source plane may not alias");
    if (((uintptr_t)d_image_inout | (uintptr_t)d_mask | (uintptr_t)d_source_or_null) & 3u)
        return fail(c, RSDSFM_ERR_INVALID, "inpaint: every plane must be 4-byte aligned");
    if ((uintptr_t)d_count_or_null & 7u) return fail(c, RSDSFM_ERR_INVALID, "inpaint: the counter must be 8-byte aligned");
    DenseWs* ws = nullptr;
    int rc = rectify_dense_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    rc = ensure_plane(c, &ws->d_inpaint, inpaint_ws_bytes(rows, cols), "inpaint: no memory for the pyramid");
    if (rc != RSDSFM_OK) return rc;
    return inpaint_launch(c, ws->d_inpaint, d_image_inout, d_mask, channels, rows, cols, d_source_or_null, d_count_or_null);
}

int rsdsfm_stabilize_video_inpainted_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                         double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                         const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows, double* const* d_depth_maps,
                                         double* const* d_R, double* const* d_t, rsdsfm_frame_result* results,
                                         const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks_or_null,
                                         const rsdsfm_link_params* link_params_or_null, rsdsfm_link_record* records, double* scales, double* A, double* c_,
                                         uint8_t* broken_or_null, const rsdsfm_fuse_params* fuse_params_or_null, double* const* d_fused_maps_or_null,
                                         const rsdsfm_stabilize_params* stabilize_params_or_null, int mode, int q5_mode, int32_t iterations, double* A_s,
                                         double* c_s, double* M, double* m, uint8_t* const* d_stab_images, uint8_t* const* d_masks_out,
                                         int64_t* valid_or_null, const rsdsfm_stabilize_fill_params* fill_params_or_null, uint8_t* const* d_sources_or_null,
                                         int64_t* counts_or_null, const rsdsfm_stabilize_crop_params* crop_params_or_null, const int32_t* window_in_or_null,
                                         uint8_t* const* d_crop_images, uint8_t* const* d_crop_masks, uint8_t* const* d_crop_sources_or_null,
                                         int32_t window_out[4], int64_t* crop_counts_or_null, const rsdsfm_stabilize_blend_params* blend_params_or_null,
                                         uint8_t* const* d_blend_images, uint8_t* const* d_blend_masks, uint8_t* const* d_blend_sources, uint32_t* gains_or_null,
                                         int64_t* blend_counts_or_null, uint8_t* const* d_inpaint_images, uint8_t* const* d_inpaint_sources_or_null,
                                         int64_t* inpaint_counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (nframes < 2) return fail(c, RSDSFM_ERR_INVALID, "stabilise video: nframes must be >= 2");
    const int np = stabilize_rendered_frames(stabilize_params_or_null, nframes);  // rendered frames: the pairs' first frames, and the last frame when asked for
    if (!all_set(d_inpaint_images, np) || (d_inpaint_sources_or_null && !all_set(d_inpaint_sources_or_null, np)))
        return fail(c, RSDSFM_ERR_INVALID, "inpaint: d_inpaint_images is required, and every plane of d_inpaint_sources when it is passed");
    for (int p = 0; p < np; ++p) {
        const uint8_t* img = d_inpaint_images[p];
        const uint8_t* src = d_inpaint_sources_or_null ? d_inpaint_sources_or_null[p] : nullptr;
        if (((uintptr_t)img | (uintptr_t)src) & 3u) return fail(c, RSDSFM_ERR_INVALID, "inpaint: inpaint images and source planes must be 4-byte aligned");
        const uint8_t* blend[3] = {d_blend_images ? d_blend_images[p] : nullptr, d_blend_masks ? d_blend_masks[p] : nullptr, d_blend_sources ? d_blend_sources[p] : nullptr};
        for (int i = 0; i < 3; ++i)
            if (img == blend[i] || (src && src == blend[i])) return fail(c, RSDSFM_ERR_INVALID, "inpaint: an inpaint plane may not be one of the frame's blend planes");
        if (img == src) return fail(c, RSDSFM_ERR_INVALID, "inpaint: a frame's inpaint planes must be distinct");
    }
    // the blended clip: the public entry point itself, so that it runs the code it runs alone (and refuses what it refuses)
    int rc = rsdsfm_stabilize_video_blended_dev(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds, d_flows,
                                                d_depth_maps, d_R, d_t, results, check_params_or_null, d_masks_or_null, link_params_or_null, records, scales, A, c_,
                                                broken_or_null, fuse_params_or_null, d_fused_maps_or_null, stabilize_params_or_null, mode, q5_mode, iterations, A_s, c_s, M,
                                                m, d_stab_images, d_masks_out, valid_or_null, fill_params_or_null, d_sources_or_null, counts_or_null, crop_params_or_null,
                                                window_in_or_null, d_crop_images, d_crop_masks, d_crop_sources_or_null, window_out, crop_counts_or_null,
                                                blend_params_or_null, d_blend_images, d_blend_masks, d_blend_sources, gains_or_null, blend_counts_or_null);
    if (rc != RSDSFM_OK) return rc;
    const size_t plane = (size_t)rows * (size_t)cols;
    DeviceCounts counts;  // with the host array: one counter per frame (every frame call zeroes its own)
    rc = counts.alloc(c, inpaint_counts_or_null != nullptr, (size_t)np);
    // without a window the blend planes are zero: the copies are, the mask has no set pixel and the frame call writes nothing
    for (int p = 0; p < np && rc == RSDSFM_OK; ++p) {
        if (hipMemcpyAsync(d_inpaint_images[p], d_blend_images[p], plane * (size_t)channels, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
            (d_inpaint_sources_or_null &&
             hipMemcpyAsync(d_inpaint_sources_or_null[p], d_blend_sources[p], plane, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)) {
            rc = fail(c, RSDSFM_ERR_HIP, "inpaint: copying the blend planes failed");
            break;
        }
        rc = rsdsfm_inpaint_frame_dev(ctx, d_inpaint_images[p], d_blend_masks[p], channels, rows, cols, d_inpaint_sources_or_null ? d_inpaint_sources_or_null[p] : nullptr,
                                      counts.at((size_t)p));
    }
    return counts.fetch(c, inpaint_counts_or_null, rc);
}

}  // extern "C"
