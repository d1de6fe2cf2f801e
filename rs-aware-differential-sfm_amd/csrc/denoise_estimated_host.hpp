// denoise_estimated_host.hpp -- what the hosts of the estimated-strength denoise share (noise_host.hip: the noise level, "auto";
// noise_curve_host.hip: the noise curve; noise_temporal_host.hip: the temporal noise curve): the arguments of a frame call and of a clip
// call as structs, the front of a frame call (every check, the top-up's workspace plane and the own render), its tail, the clip call, and the
// refusals that differ between the stages in one noun.  A stage keeps what it alone does: its estimator's parameters, its workspace planes
// and the middle of its frame call -- measure, then accumulate.  DESIGN section 12, "Estimated-strength denoise: one frame skeleton".
#pragma once

#include <stdint.h>

#include <initializer_list>
#include <vector>

#include "clip_stage_host.hpp"
#include "denoise.hpp"
#include "rectify_dense.hpp"

namespace rsdsfm {

// "<stage>: <what>" as RSDSFM_ERR_INVALID
int stage_fail(Ctx* c, const char* stage, const char* what);

// An estimate a call reads or writes -- noun: "noise record", "noise curve" -- given, 8-byte aligned and none of `outputs` (NULL entries are
// skipped); RSDSFM_OK, or the refusal "<stage>: ..."
int estimate_check(Ctx* c, const char* stage, const char* noun, const uint64_t* d_estimate, std::initializer_list<const void*> outputs);
// What a primitive that measures a frame refuses about its planes, its histogram and its estimate -- noun: "record", "curve"
int measure_planes_check(Ctx* c, const char* stage, const char* noun, const uint8_t* d_image, const uint8_t* d_mask, int channels, int rows, int cols, const uint32_t* d_hist,
                         const uint64_t* d_estimate);

// The arguments of a frame call, the estimator's parameters aside; d_estimate_or_null: where the caller wants the record or the curve
struct EstimatedFrame {
    const uint8_t* const* d_images;
    int32_t channels;
    const double *const *d_depths_colmajor, *const *d_R_rows9, *const *d_t_rows3;
    double fx, fy, cx, cy;
    int32_t rows, cols;
    int mode, q5_mode;
    int32_t iterations, nsrc;
    const double *M, *m;
    const rsdsfm_denoise_params* params_or_null;
    const rsdsfm_denoise_spatial_params* spatial_or_null;
    const int32_t* window_or_null;
    uint8_t *d_image_out, *d_mask_out, *d_weight_or_null, *d_support_or_null;
    int64_t* d_counts6_or_null;
    uint64_t* d_estimate_or_null;
};

// What the front hands to the middle of a frame call.  `window` may point into `full`: filled in place, not copied
struct EstimatedFront {
    rsdsfm_denoise_params dp;
    rsdsfm_denoise_spatial_params sp;
    bool top_up;  // the top-up's parameters were passed
    RenderGeom g;
    DenoisePlanes r;  // the reference is rendered
    int32_t full[4];
    const int32_t* window;
    DenseWs* ws;
    // the temporal stage's outputs: with the top-up its image (and its weight, when the caller has no plane for it) stay in the workspace
    uint8_t *d_image, *d_weight;
    int64_t* d_counts3;    // the top-up's three counters, or NULL
    uint64_t* d_estimate;  // the caller's buffer, else the workspace's
};

// The front of a frame call, in two parts around the stage's own workspace planes.  estimated_checks, in this order: rectify_dense_check, nsrc,
// the denoise's parameters, estimator_refusal, the top-up's parameters, a support plane without them, the sources, the poses, the output
// planes, the estimate output (noun: "noise record"; aligned, none of the outputs, none of the 4 nsrc source pointers), the window; then
// front->ws.  estimator_refusal: the stage resolves its own parameters BEFORE this call (the resolve has no side effect) and passes
// the whole message of a failed resolve, or NULL; it is reported here, at its place in the order, so a stage must not use its resolved
// parameters before this call has returned RSDSFM_OK.
int estimated_checks(rsdsfm_ctx* ctx, const char* stage, const char* noun, const EstimatedFrame& a, const char* estimator_refusal, EstimatedFront* front);
// Behind the stage's planes (DenseWs::d_denoise among them, ensured in the stage's order under the stage's "no memory" messages): the top-up's
// plane, the routed outputs, d_estimate (d_estimate_ws: the workspace's place for it), what the top-up would refuse -- all of it still in
// front of anything enqueued -- then the own render onto front->r
int estimated_render(rsdsfm_ctx* ctx, const char* stage, const EstimatedFrame& a, uint64_t* d_estimate_ws, EstimatedFront* front);
// The tail of a frame call without the top-up: its three counters are 0.  (With it the stage's last line is its own top-up call.)
int estimated_tail(Ctx* c, const EstimatedFront& front);

// The arguments of a clip call, the estimator's parameters aside; estimates_or_null: `words` host words per frame
struct EstimatedClip {
    const uint8_t* const* d_frames;
    int32_t nsources, rows, cols, channels;
    double fx, fy, cx, cy;
    const double *const *d_depth_maps, *const *d_R, *const *d_t;
    const double *A, *c_, *A_path, *c_path, *scales;
    int mode, q5_mode;
    int32_t iterations;
    const rsdsfm_denoise_params* params_or_null;
    const rsdsfm_denoise_spatial_params* spatial_or_null;
    const int32_t* window_or_null;
    uint8_t *const *d_out_images, *const *d_out_masks, *const *d_out_weights_or_null, *const *d_out_supports_or_null;
    int64_t* counts_or_null;
    uint64_t* estimates_or_null;
};

// The clip call: the clip's arrays, the three parameter checks (estimator_refusal as above), the supports without the top-up's parameters,
// then the walk with frame_call(const EstimatedFrame&) per frame on 6 + words device words, [counts: 6][estimate: words], when the caller
// asks for either: one copy and one wait for both
template <class FrameCall>
int estimated_clip(rsdsfm_ctx* ctx, const char* stage, const EstimatedClip& a, const char* estimator_refusal, int words, FrameCall frame_call) {
    Ctx* c = &ctx->c;
    ClipOutputs outs;
    outs.planes[0] = a.d_out_images;
    outs.planes[1] = a.d_out_masks;
    outs.planes[2] = a.d_out_weights_or_null;
    outs.planes[3] = a.d_out_supports_or_null;
    int rc = clip_arrays_check(c, stage, a.d_frames, a.nsources, a.d_depth_maps, a.d_R, a.d_t, a.A, a.c_, a.A_path, a.c_path, a.scales, outs,
                               "its weight and support planes when the arrays are passed");
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_denoise_params dp;  // the radius of the walk is the temporal stage's
    if (!denoise_params_resolve(a.params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDenoiseParamsMessage);
    if (estimator_refusal) return fail(c, RSDSFM_ERR_INVALID, estimator_refusal);
    rsdsfm_denoise_spatial_params sp;
    if (!spatial_params_resolve(a.spatial_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kSpatialParamsMessage);
    if (a.d_out_supports_or_null && !a.spatial_or_null) return stage_fail(c, stage, "the support planes need the top-up's parameters");
    const int per_frame = 6 + words;
    const bool wanted = a.counts_or_null || a.estimates_or_null;
    std::vector<int64_t> host(wanted ? (size_t)per_frame * (size_t)a.nsources : 0);
    rc = walk_clip(c, stage, a.d_frames, a.nsources, a.d_depth_maps, a.d_R, a.d_t, a.A, a.c_, a.A_path, a.c_path, a.scales, dp.radius, outs, per_frame,
                   wanted ? host.data() : nullptr, [&](const ClipFrame& f) {
                       return frame_call(EstimatedFrame{f.img, a.channels, f.map, f.R, f.t, a.fx, a.fy, a.cx, a.cy, a.rows, a.cols, a.mode, a.q5_mode, a.iterations, f.plan->nsrc,
                                                        f.plan->M, f.plan->m, a.params_or_null, a.spatial_or_null, a.window_or_null, f.out[0], f.out[1], f.out[2], f.out[3], f.d_counts,
                                                        f.d_counts ? reinterpret_cast<uint64_t*>(f.d_counts + 6) : nullptr});
                   });
    if (rc != RSDSFM_OK || !wanted) return rc;
    for (int q = 0; q < a.nsources; ++q) {
        const int64_t* w = host.data() + (size_t)per_frame * (size_t)q;
        for (int k = 0; k < 6 && a.counts_or_null; ++k) a.counts_or_null[6 * (size_t)q + k] = w[k];
        for (int k = 0; k < words && a.estimates_or_null; ++k) a.estimates_or_null[(size_t)words * (size_t)q + k] = (uint64_t)w[6 + k];
    }
    return RSDSFM_OK;
}

}  // namespace rsdsfm
