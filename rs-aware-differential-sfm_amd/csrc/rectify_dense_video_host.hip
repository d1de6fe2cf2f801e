// rectify_dense_video_host.hip -- rsdsfm_rectify_dense_video_dev (include/rsdsfm_rectify_dense.h): rsdsfm_solve_video_dev's batch loop
// (flow_seq_host.hip: solve_video_run) with a hook behind every pair's solve that enqueues the dense rectification of frame p on the pair's
// LANE, with that lane's pyramid and displacement plane -- built as rectify_video_host.hip builds the splat's clip call.  The lane's next
// solve is enqueued behind it on the same stream, so a lane-owned pose table is read before it is overwritten.  No kernel of its own.
#include "../../include/rsdsfm_rectify_dense.h"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"

using namespace rsdsfm;

extern "C" {

int rsdsfm_rectify_dense_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                   double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                   const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows_or_null,
                                   double* const* d_depth_maps, double* const* d_R_or_null, double* const* d_t_or_null, rsdsfm_frame_result* results,
                                   int mode, int q5_mode, int32_t iterations, uint8_t* const* d_dense_images, uint8_t* const* d_masks_or_null,
                                   double* const* d_filled_depths_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (nframes < 2) return fail(c, RSDSFM_ERR_INVALID, "rectify video: nframes must be >= 2");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "rectify video: channels must be 1 or 3");
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    const int np = nframes - 1;
    if (!all_set(d_dense_images, np) || (d_masks_or_null && !all_set(d_masks_or_null, np)) || (d_filled_depths_or_null && !all_set(d_filled_depths_or_null, np)))
        return fail(c, RSDSFM_ERR_INVALID, "rectify video: null device pointer");
    for (int p = 0; p < np; ++p) {
        if (d_frames && d_dense_images[p] == d_frames[p]) return fail(c, RSDSFM_ERR_INVALID, "rectify video: a pair's output image is its frame");
        if (((uintptr_t)d_dense_images[p] | (uintptr_t)(d_masks_or_null ? d_masks_or_null[p] : nullptr)) & 3u)
            return fail(c, RSDSFM_ERR_INVALID, "dense rectifier: images and mask must be 4-byte aligned");
    }
    const int it = iterations ? iterations : 3;
    const PairHook rectify = [&](Ctx* lane, int p, const rsdsfm_frame_job& job, const rsdsfm_frame_result&) -> int {
        DenseWs* ws = nullptr;
        int rc2 = rectify_dense_ws(lane, rows, cols, &ws);
        if (rc2 != RSDSFM_OK) return rc2;
        return rectify_dense_launch(lane, *ws, d_frames[p], channels, job.d_depth_map_colmajor, job.d_R_rows9_or_null, job.d_t_rows3_or_null, fx, fy, cx, cy, rows,
                                    cols, mode, q5_mode, it, d_dense_images[p], d_masks_or_null ? d_masks_or_null[p] : nullptr,
                                    d_filled_depths_or_null ? d_filled_depths_or_null[p] : nullptr);
    };
    rc = solve_video_run(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds, d_flows_or_null, d_depth_maps,
                         d_R_or_null, d_t_or_null, results, &rectify, true);
    // every output is complete when the call returns (and nothing reads a caller's buffer after an error): wait for every lane's rectifier
    int rc_wait = RSDSFM_OK;
    if (hipStreamSynchronize(c->stream) != hipSuccess) rc_wait = RSDSFM_ERR_HIP;
    for (rsdsfm_ctx* lane : c->lanes)
        if (hipStreamSynchronize(lane->c.stream) != hipSuccess) rc_wait = RSDSFM_ERR_HIP;
    if (rc != RSDSFM_OK) return rc;
    return rc_wait == RSDSFM_OK ? RSDSFM_OK : fail(c, rc_wait, "rectify video: a lane's stream failed");
}

}  // extern "C"
