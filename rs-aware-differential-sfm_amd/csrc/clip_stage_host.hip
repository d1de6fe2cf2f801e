// clip_stage_host.hip -- clip_stage_host.hpp's out-of-line part: one frame's plan, the render choice, the device counters and the clip walk.
#include "clip_stage_host.hpp"

#include <string>
#include <vector>

#include "../../include/rsdsfm_retime.h"
#include "../../include/rsdsfm_stabilize_crop.h"
#include "../../include/rsdsfm_stabilize_fill.h"
#include "../../include/rsdsfm_stabilize_search.h"
#include "../../include/rsdsfm_stabilize_visible.h"
#include "sequence_host.hpp"

namespace rsdsfm {

namespace {

int fail_at(Ctx* c, int code, const char* stage, const char* what) { return fail(c, code, (std::string(stage) + ": " + what).c_str()); }

}  // namespace

bool clip_plan(const double* A, const double* c_, const double* A_path, const double* c_path, const double* scales, int nsources, int q, int radius, ClipPlan* plan) {
    int32_t src2[2], nsrc = 0, wq = 0, ids[kClipSourcesMax - 1], count = 0;
    double M18[18], m6[6], At[9], ct[3];
    if (rsdsfm_retime_poses(A, c_, A_path, c_path, scales, nsources, (double)q, src2, &nsrc, &wq, M18, m6, At, ct) != RSDSFM_OK || nsrc != 1) return false;
    plan->src[0] = q;
    for (int k = 0; k < 9; ++k) plan->M[k] = M18[k];
    for (int k = 0; k < 3; ++k) plan->m[k] = m6[k];
    if (nsources > 1 && rsdsfm_neighbour_poses(A, c_, A_path, c_path, scales, nsources, q, radius, plan->src + 1, ids, plan->M + 9, plan->m + 3, &count) != RSDSFM_OK)
        return false;
    plan->nsrc = 1 + count;
    return finite_all(plan->M, 9 * plan->nsrc) && finite_all(plan->m, 3 * plan->nsrc);
}

int render_candidate(rsdsfm_ctx* ctx, bool occlusion, int tol_q16, const uint8_t* d_image_n, int channels, const double* d_depth_n, const double* d_R_n, const double* d_t_n,
                     double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const double* M9, const double* m3, int id,
                     const int32_t* window, uint8_t* d_image, uint8_t* d_mask, uint8_t* d_source_or_null, int64_t* d_counts_or_null) {
    if (occlusion && ctx->c.occlusion_search == 1)
        return rsdsfm_stabilize_search_frame_dev(ctx, d_image_n, channels, d_depth_n, d_R_n, d_t_n, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, M9, m3, id, window,
                                                 d_image, d_mask, d_source_or_null, tol_q16, d_counts_or_null);
    if (occlusion)
        return rsdsfm_stabilize_visible_frame_dev(ctx, d_image_n, channels, d_depth_n, d_R_n, d_t_n, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, M9, m3, id, window,
                                                  d_image, d_mask, d_source_or_null, tol_q16, d_counts_or_null);
    return rsdsfm_stabilize_window_frame_dev(ctx, d_image_n, channels, d_depth_n, d_R_n, d_t_n, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, M9, m3, id, window,
                                             d_image, d_mask, d_source_or_null, d_counts_or_null);
}

int render_reference(rsdsfm_ctx* ctx, const char* stage, const uint8_t* d_image_n, int channels, const double* d_depth_n, const double* d_R_n, const double* d_t_n, double fx,
                     double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const double* M9, const double* m3, const int32_t* window,
                     uint8_t* d_rimage, uint8_t* d_rmask, uint8_t* d_rsource) {
    Ctx* c = &ctx->c;
    const size_t plane = (size_t)rows * (size_t)cols;
    if (hipMemsetAsync(d_rimage, 0, plane * (size_t)channels, c->stream) != hipSuccess || hipMemsetAsync(d_rmask, 0, plane, c->stream) != hipSuccess ||
        hipMemsetAsync(d_rsource, 0, plane, c->stream) != hipSuccess)
        return fail_at(c, RSDSFM_ERR_HIP, stage, "zeroing the reference failed");
    return rsdsfm_stabilize_window_frame_dev(ctx, d_image_n, channels, d_depth_n, d_R_n, d_t_n, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, M9, m3, 1, window,
                                             d_rimage, d_rmask, d_rsource, nullptr);
}

int DeviceCounts::alloc(Ctx* c, bool wanted, size_t n, bool zero) {
    if (!wanted) return RSDSFM_OK;
    RSDSFM_HIP_CHECK(c, hipMalloc(reinterpret_cast<void**>(&d_), sizeof(int64_t) * n));
    n_ = n;
    if (zero) {
        const hipError_t e = hipMemsetAsync(d_, 0, sizeof(int64_t) * n, c->stream);
        if (e != hipSuccess) {
            release();
            RSDSFM_HIP_CHECK(c, e);
        }
    }
    return RSDSFM_OK;
}

int DeviceCounts::fetch(Ctx* c, int64_t* host, int rc) {
    if (!d_) return rc;
    hipError_t e = rc == RSDSFM_OK ? hipMemcpyAsync(host, d_, sizeof(int64_t) * n_, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    release();
    if (rc == RSDSFM_OK) RSDSFM_HIP_CHECK(c, e);
    return rc;
}

void DeviceCounts::release() {
    if (d_) (void)hipFree(d_);
    d_ = nullptr;
    n_ = 0;
}

int clip_arrays_check(Ctx* c, const char* stage, const uint8_t* const* d_frames, int nsources, const double* const* d_depth_maps, const double* const* d_R,
                      const double* const* d_t, const double* A, const double* c_, const double* A_path, const double* c_path, const double* scales,
                      const ClipOutputs& outputs, const char* optional_note) {
    if (nsources < 1) return fail_at(c, RSDSFM_ERR_INVALID, stage, "nsources must be >= 1");
    if (!d_frames || !d_depth_maps || !d_R || !d_t || !A || !c_ || !A_path || !c_path || !scales) return fail_at(c, RSDSFM_ERR_INVALID, stage, "null array");
    if (!all_set(d_frames, nsources) || !all_set(d_depth_maps, nsources) || !all_set(d_R, nsources) || !all_set(d_t, nsources))
        return fail_at(c, RSDSFM_ERR_INVALID, stage, "every source needs its frame, depth map and pose table");
    bool given = all_set(outputs.planes[0], nsources) && all_set(outputs.planes[1], nsources);
    for (int k = 2; k < 4; ++k) given = given && (!outputs.planes[k] || all_set(outputs.planes[k], nsources));
    if (!given) return fail_at(c, RSDSFM_ERR_INVALID, stage, (std::string("every frame needs its image and its mask (and ") + optional_note + ")").c_str());
    return RSDSFM_OK;
}

int clip_plans(Ctx* c, const char* stage, const uint8_t* const* d_frames, int nsources, const double* A, const double* c_, const double* A_path, const double* c_path,
               const double* scales, int radius, const ClipOutputs& outputs, std::vector<ClipPlan>* plans) {
    for (int q = 0; q < nsources; ++q)  // an output may not be a frame of the clip: a later frame call still reads it
        for (int n = 0; n < nsources; ++n)
            for (int k = 0; k < 4; ++k)
                if (outputs.planes[k] && d_frames[n] == outputs.planes[k][q]) return fail_at(c, RSDSFM_ERR_INVALID, stage, "an output plane may not be a frame of the clip");
    // every frame's sources and poses first: a refused pose enqueues nothing
    plans->resize(nsources);
    for (int q = 0; q < nsources; ++q)
        if (!clip_plan(A, c_, A_path, c_path, scales, nsources, q, radius, &(*plans)[q]))
            return fail_at(c, RSDSFM_ERR_INVALID, stage, "the poses must be finite and every listed source's scale finite and positive");
    return RSDSFM_OK;
}

ClipFrame clip_frame(const ClipPlan& plan, const uint8_t* const* d_frames, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t,
                     const ClipOutputs& outputs, int q, int64_t* d_counts) {
    ClipFrame f;
    f.plan = &plan;
    for (int k = 0; k < plan.nsrc; ++k) {
        const int n = plan.src[k];
        f.img[k] = d_frames[n];
        f.map[k] = d_depth_maps[n];
        f.R[k] = d_R[n];
        f.t[k] = d_t[n];
    }
    for (int k = 0; k < 4; ++k) f.out[k] = outputs.planes[k] ? outputs.planes[k][q] : nullptr;
    f.d_counts = d_counts;
    return f;
}

}  // namespace rsdsfm
