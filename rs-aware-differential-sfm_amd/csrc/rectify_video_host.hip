// rectify_video_host.hip -- rsdsfm_rectify_video_dev (include/rsdsfm_rectify_video.h): main.cc:380-523 for a whole clip.  It is
// rsdsfm_solve_video_dev's batch loop (flow_seq_host.hip: solve_video_run) with a hook behind every pair's solve that enqueues the pair's
// rectification (rectify_kernels.hip; its gray twin for one channel) on the pair's LANE: the lane context's claim maps and workspace, as
// rsdsfm_rectify_frame_dev behind rsdsfm_solve_frame_dev uses a single context's.  The lane's next solve is enqueued behind it on the same
// stream, so the pair's device inlier list (and a lane-owned pose table) is read before it is overwritten.  No kernel of its own.
#include "../../include/rsdsfm_rectify_video.h"
#include "rectify_gray.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"

using namespace rsdsfm;

extern "C" {

int rsdsfm_rectify_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels, double fx,
                             double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                             const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows_or_null, double* const* d_depth_maps,
                             double* const* d_R_or_null, double* const* d_t_or_null, rsdsfm_frame_result* results, int mode, int q5_mode, int32_t offset,
                             uint8_t* const* d_depth_est, uint8_t* const* d_gs_images, uint8_t* const* d_fixed_images, float* const* d_coords3d_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (nframes < 2) return fail(c, RSDSFM_ERR_INVALID, "rectify video: nframes must be >= 2");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "rectify video: channels must be 1 or 3");
    if (mode != RSDSFM_BACKPROJECT_RS && mode != RSDSFM_BACKPROJECT_GS) return fail(c, RSDSFM_ERR_INVALID, "unknown back-projection mode");
    if (q5_mode != RSDSFM_Q5_COMPAT && q5_mode != RSDSFM_Q5_FIXED) return fail(c, RSDSFM_ERR_INVALID, "unknown q5_mode");
    if (offset < 0) return fail(c, RSDSFM_ERR_INVALID, "rectify video: negative interpolation offset");
    const int np = nframes - 1;
    if (!all_set(d_depth_est, np) || !all_set(d_gs_images, np) || !all_set(d_fixed_images, np) || (d_coords3d_or_null && !all_set(d_coords3d_or_null, np)))
        return fail(c, RSDSFM_ERR_INVALID, "rectify video: null device pointer");
    for (int p = 0; p < np; ++p)
        if (d_gs_images[p] == d_fixed_images[p]) return fail(c, RSDSFM_ERR_INVALID, "rectify video: a pair's two output images are one buffer");
    for (int p = 0; p < np; ++p)  // as rsdsfm_rectify_frame_dev (the depth images: any address; the solve's own buffers: solve_video_run)
        if (!aligned_to(4, d_gs_images[p], d_fixed_images[p], d_coords3d_or_null ? d_coords3d_or_null[p] : nullptr) || (d_frames && !aligned_to(4, d_frames[p], d_frames[p + 1])))
            return fail(c, RSDSFM_ERR_INVALID, "rectify video: every image buffer and the world points must be 4-byte aligned");
    const PairHook rectify = [&](Ctx* lane, int p, const rsdsfm_frame_job& job, const rsdsfm_frame_result& r) -> int {
        int rc = ensure_ws(lane, Arena::need(8 * 2048) + 1024);
        if (rc != RSDSFM_OK) return rc;
        return (channels == 1 ? rectify_gray_frame_launch : rectify_frame_launch)(
            lane, r.d_inliers, r.num_inliers, d_frames[p], job.d_depth_map_colmajor, job.d_R_rows9_or_null, job.d_t_rows3_or_null, fx, fy, cx, cy, rows, cols, mode,
            q5_mode, offset, d_depth_est[p], d_gs_images[p], d_coords3d_or_null ? d_coords3d_or_null[p] : nullptr, d_fixed_images[p], static_cast<double*>(lane->d_ws));
    };
    const int rc = solve_video_run(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds, d_flows_or_null,
                                   d_depth_maps, d_R_or_null, d_t_or_null, results, &rectify, true);
    // every output is complete when the call returns (and nothing reads a caller's buffer after an error): wait for every lane's rectifier
    int rc_wait = RSDSFM_OK;
    if (hipStreamSynchronize(c->stream) != hipSuccess) rc_wait = RSDSFM_ERR_HIP;
    for (rsdsfm_ctx* lane : c->lanes)
        if (hipStreamSynchronize(lane->c.stream) != hipSuccess) rc_wait = RSDSFM_ERR_HIP;
    if (rc != RSDSFM_OK) return rc;
    return rc_wait == RSDSFM_OK ? RSDSFM_OK : fail(c, rc_wait, "rectify video: a lane's stream failed");
}

}  // extern "C"
