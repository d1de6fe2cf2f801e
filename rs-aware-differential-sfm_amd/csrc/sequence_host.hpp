// sequence_host.hpp -- the drivers behind rsdsfm_solve_frames_dev (frame_host.hip) and rsdsfm_solve_video_dev (flow_seq_host.hip) with a
// per-pair hook, for callers that put work of their own behind every pair's solve (rectify_video_host.hip: the clip rectifier).
#pragma once

#include <stdint.h>

#include <functional>

#include "../../include/rsdsfm_flow.h"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace flowhost {
struct FlowWs;
}

// Called right after pair `pair` has been finished on its lane (`lane`: the lane's context; results[pair] is complete, its device
// pointers are valid) and before that lane begins its next pair: what the hook enqueues on lane->stream runs in front of the lane's next
// solve, which overwrites the pair's device inlier list.  `job` is the pair's job.  An error ends the sequence like an error of the solve.
using PairHook = std::function<int(Ctx* lane, int pair, const rsdsfm_frame_job& job, const rsdsfm_frame_result& result)>;

// Called once per batch of a clip, after the batch's fields have been enqueued on the context's stream and before its solve: `fields`
// are the n device fields of pairs g0 .. g0 + n - 1 (the caller's buffers or the ring), `w` the clip workspace they were computed on, `p`
// the flow parameters in use.  What the hook enqueues on the context's stream runs between the flow and the solve (flow_check_host.hip: the
// backward fields and the forward-backward check, which masks `fields` in place).  An error ends the clip.
using BatchHook = std::function<int(const flowhost::FlowWs* w, const rsdsfm_flow_params& p, int g0, int n, double* const* fields)>;

// lanes a sequence of `count` pairs runs on (pair i on lane i % L; lane 0 is the context itself, lane l > 0 is c->lanes[l - 1])
int sequence_lane_count(const Ctx* c, int count);

// pairs per batch of the clip calls on this context (rsdsfm_set_flow_batch, or the default): the clip workspace's B
int video_batch_size(const Ctx* c);

// rsdsfm_solve_frames_dev behind its argument check (count >= 1); hook NULL = that call exactly
int solve_frames_run(Ctx* c, const rsdsfm_frame_job* jobs, int32_t count, const rsdsfm_frame_params* prm, rsdsfm_frame_result* results, const PairHook* hook);

// rsdsfm_solve_video_dev (its arguments, its checks, its batch loop); the hook numbers the pairs within the clip.  lane_tables: with a
// hook, every pair whose d_R_or_null / d_t_or_null entry is missing gets its lane's scratch table (rows x 9 / rows x 3 doubles, owned
// by the clip workspace) in its job, so that the hook finds the pair's pose table either way.  pre_solve NULL = no work between a batch's
// flow and its solve.
int solve_video_run(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                    double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null, const rsdsfm_frame_params* params,
                    const uint64_t* seeds, double* const* d_flows_or_null, double* const* d_depth_maps, double* const* d_R_or_null,
                    double* const* d_t_or_null, rsdsfm_frame_result* results, const PairHook* hook, bool lane_tables,
                    const BatchHook* pre_solve = nullptr);

// no NULL among the n pointers of a required array
template <class T>
inline bool all_set(T* const* a, int n) {
    if (!a) return false;
    for (int i = 0; i < n; ++i)
        if (!a[i]) return false;
    return true;
}

}  // namespace rsdsfm
