// flow_seq_host.hip -- C ABI of whole clips (include/rsdsfm_video.h; Camera::calculateDeepFlow, camera.cc:253-277, for every
// consecutive pair, and the solve of main.cc:380-457 per pair; DESIGN section 12, "Sequences").  A clip is cut into batches of up to
// B pairs; each goes through the level loop of flow_host.hip on the context's clip workspace (the batched kernels of
// flow_seq_kernels.hip, at B = 1 too).
#include <algorithm>
#include <string>

#include "../../include/rsdsfm_video.h"
#include "flow_host.hpp"
#include "flow_kernels.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"

namespace rsdsfm {
namespace {

using namespace flowhost;

constexpr int kFlowBatchDefault = 8;  // profiles/flow_seq_time.txt

// the context's clip workspace, ready for this size and pyramid at the batch size of rsdsfm_set_flow_batch
int clip_ws(Ctx* c, int rows, int cols, const rsdsfm_flow_params& p, FlowWs** w) {
    *w = flow_ws(c, false);
    return ensure_flow_ws(c, *w, video_batch_size(c), rows, cols, p);
}

// the ring of B fields behind rsdsfm_solve_video_dev's d_flows_or_null = NULL (freed with the workspace)
int ensure_ring(Ctx* c, FlowWs* w) {
    if (w->d_ring) return RSDSFM_OK;
    w->ring_stride = Arena::need(16 * (size_t)w->rows * w->cols);
    RSDSFM_HIP_CHECK(c, hipMalloc(&w->d_ring, (size_t)w->B * w->ring_stride));
    return RSDSFM_OK;
}

// the lanes' scratch pose tables behind rsdsfm_rectify_video_dev's d_R_or_null / d_t_or_null = NULL (freed with the workspace)
int ensure_tables(Ctx* c, FlowWs* w) {
    if (w->d_tables) return RSDSFM_OK;
    RSDSFM_HIP_CHECK(c, hipMalloc(reinterpret_cast<void**>(&w->d_tables), sizeof(double) * 12 * (size_t)w->rows * kLaneTables));
    return RSDSFM_OK;
}

int check_clip(Ctx* c, int nframes, int rows, int cols, int channels, const rsdsfm_flow_params* pp, rsdsfm_flow_params* p) {
    int rc = check_args(c, rows, cols, channels, pp, p);
    if (rc != RSDSFM_OK) return rc;
    if (nframes < 2) return fail(c, RSDSFM_ERR_INVALID, "deep flow sequence: nframes must be >= 2");
    return RSDSFM_OK;
}

}  // namespace

int video_batch_size(const Ctx* c) { return c->flow_batch > 0 ? c->flow_batch : kFlowBatchDefault; }

int solve_video_run(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                    double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null, const rsdsfm_frame_params* params,
                    const uint64_t* seeds, double* const* d_flows_or_null, double* const* d_depth_maps, double* const* d_R_or_null,
                    double* const* d_t_or_null, rsdsfm_frame_result* results, const PairHook* hook, bool lane_tables, const BatchHook* pre_solve) {
    Ctx* c = &ctx->c;
    rsdsfm_flow_params p;
    int rc = check_clip(c, nframes, rows, cols, channels, flow_params_or_null, &p);
    if (rc != RSDSFM_OK) return rc;
    const int np = nframes - 1;
    if (!params || !results) return fail(c, RSDSFM_ERR_INVALID, "solve video: bad arguments");
    if (!all_set(d_frames, nframes) || !all_set(d_depth_maps, np) || (d_flows_or_null && !all_set(d_flows_or_null, np)) ||
        (d_R_or_null && !all_set(d_R_or_null, np)) || (d_t_or_null && !all_set(d_t_or_null, np)))
        return fail(c, RSDSFM_ERR_INVALID, "solve video: null device pointer");
    // what becomes a pair's rsdsfm_frame_job (frame_host.hip: frame_begin holds every job to this) is checked for the whole clip before the
    // first batch's flow is enqueued
    for (int q = 0; q < np; ++q)
        if (!aligned_to(16, d_flows_or_null ? d_flows_or_null[q] : nullptr) ||
            !aligned_to(8, d_depth_maps[q], d_R_or_null ? d_R_or_null[q] : nullptr, d_t_or_null ? d_t_or_null[q] : nullptr))
            return fail(c, RSDSFM_ERR_INVALID, "solve video: the flow fields must be 16-byte aligned, the depth maps and the pose tables 8-byte aligned");
    FlowWs* w = nullptr;
    rc = clip_ws(c, rows, cols, p, &w);
    if (rc == RSDSFM_OK && !d_flows_or_null) rc = ensure_ring(c, w);
    const bool tables = hook && lane_tables && (!d_R_or_null || !d_t_or_null);
    if (rc == RSDSFM_OK && tables) rc = ensure_tables(c, w);
    if (rc != RSDSFM_OK) return rc;
    const int B = w->B;
    double* fl[kFlowSeqMaxPairs];
    rsdsfm_frame_job jobs[kFlowSeqMaxPairs];
    for (int g0 = 0; g0 < np; g0 += B) {
        const int n = std::min(B, np - g0);
        for (int q = 0; q < n; ++q)
            fl[q] = d_flows_or_null ? d_flows_or_null[g0 + q] : reinterpret_cast<double*>(static_cast<char*>(w->d_ring) + (size_t)q * w->ring_stride);
        rc = flow_enqueue(c, w, d_frames + g0, n, channels, p, fl);
        if (rc == RSDSFM_OK && pre_solve) rc = (*pre_solve)(w, p, g0, n, fl);
        if (rc != RSDSFM_OK) return rc;
        const int L = sequence_lane_count(c, n);
        for (int q = 0; q < n; ++q) {
            // (a lane's table is read by the hook's work on that lane's stream and written by the lane's next solve behind it)
            double* lane_R = tables ? w->d_tables + (size_t)(q % L) * 12 * (size_t)rows : nullptr;
            jobs[q] = rsdsfm_frame_job{fl[q], rows, cols, fx, fy, cx, cy, gamma, d_depth_maps[g0 + q], d_R_or_null ? d_R_or_null[g0 + q] : lane_R,
                                       d_t_or_null ? d_t_or_null[g0 + q] : (lane_R ? lane_R + 9 * (size_t)rows : nullptr),
                                       seeds ? seeds[g0 + q] : params->seed};
        }
        const PairHook in_clip = [&](Ctx* lane, int pair, const rsdsfm_frame_job& job, const rsdsfm_frame_result& r) { return (*hook)(lane, g0 + pair, job, r); };
        rc = solve_frames_run(c, jobs, n, params, results + g0, hook ? &in_clip : nullptr);
        if (rc != RSDSFM_OK) {
            // the pairs of the batch are numbered from 0: number them within the clip
            const size_t colon = c->err.find(':');
            if (g0 > 0 && c->err.compare(0, 5, "pair ") == 0 && colon != std::string::npos)
                c->err = "pair " + std::to_string(g0 + std::stoi(c->err.substr(5, colon - 5))) + c->err.substr(colon);
            return rc;
        }
        for (int i = 0; i < g0; ++i) results[i].d_inliers = nullptr, results[i].d_inlier_idx = nullptr, results[i].d_scanline = nullptr;
    }
    return RSDSFM_OK;
}

}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_deep_flow_seq_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                             const rsdsfm_flow_params* params_or_null, double* const* d_flows) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    rsdsfm_flow_params p;
    int rc = check_clip(c, nframes, rows, cols, channels, params_or_null, &p);
    if (rc != RSDSFM_OK) return rc;
    if (!all_set(d_frames, nframes) || !all_set(d_flows, nframes - 1)) return fail(c, RSDSFM_ERR_INVALID, "deep flow sequence: null device pointer");
    FlowWs* w = nullptr;
    rc = clip_ws(c, rows, cols, p, &w);
    for (int g0 = 0; rc == RSDSFM_OK && g0 < nframes - 1; g0 += w->B)
        rc = flow_enqueue(c, w, d_frames + g0, std::min(w->B, nframes - 1 - g0), channels, p, d_flows + g0);
    return rc;
}

int rsdsfm_deep_flow_seq(rsdsfm_ctx* ctx, const uint8_t* const* frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                         const rsdsfm_flow_params* params_or_null, double* const* flows) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    rsdsfm_flow_params p;
    int rc = check_clip(c, nframes, rows, cols, channels, params_or_null, &p);
    if (rc != RSDSFM_OK) return rc;
    if (!all_set(frames, nframes) || !all_set(flows, nframes - 1)) return fail(c, RSDSFM_ERR_INVALID, "deep flow sequence: null pointer");
    FlowWs* w = nullptr;
    rc = clip_ws(c, rows, cols, p, &w);
    if (rc != RSDSFM_OK) return rc;
    return flow_staged(c, w, frames, nframes, channels, p, flows);
}

int rsdsfm_set_flow_batch(rsdsfm_ctx* ctx, int32_t pairs) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    if (pairs < 0 || pairs > kFlowSeqMaxPairs) return fail(c, RSDSFM_ERR_INVALID, "flow batch: pairs must be 0 (default) .. 32");
    c->flow_batch = pairs;  // (the clip workspace follows on its next use)
    return RSDSFM_OK;
}

int rsdsfm_solve_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels, double fx,
                           double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                           const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows_or_null, double* const* d_depth_maps,
                           double* const* d_R_or_null, double* const* d_t_or_null, rsdsfm_frame_result* results) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    DeviceGuard device_guard_(&ctx->c);
    return solve_video_run(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds, d_flows_or_null,
                           d_depth_maps, d_R_or_null, d_t_or_null, results, nullptr, false);
}

}  // extern "C"
