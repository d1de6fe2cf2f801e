/*
 * rsdsfm_video.h -- C ABI of whole clips on the MI355X: consecutive 8-bit frames -> the DeepFlow field of every consecutive pair
 * (include/rsdsfm_flow.h) -> the solve of every pair (rsdsfm_solve_frames_dev).
 *
 * The reference runs Camera::calculateDeepFlow (camera.cc:253-277) and evaluateSingleRun's solve (main.cc:380-457) on one pair per
 * process run.  Here a clip of F frames is F - 1 pairs, processed in batches of up to B pairs: every kernel launch of the flow serves
 * every pair of its batch, and each frame's gray image and pyramid are built once per batch.  Pair p is (frame p, frame p + 1).
 * The batch size is scheduling only: every field is bit for bit what rsdsfm_deep_flow_dev computes for that pair, at every B.
 * DESIGN.md section 12 ("Sequences") describes the layout and the measured times.
 */
#ifndef RSDSFM_VIDEO_H
#define RSDSFM_VIDEO_H

#include "rsdsfm_flow.h"

#ifdef __cplusplus
extern "C" {
#endif

/* camera.cc:253-277 for every consecutive pair of a clip (main.cc:380-457 per pair), on device buffers: d_frames[0 .. nframes-1]
 * rows x cols x channels bytes each, d_flows[0 .. nframes-2] rows x cols x 2 doubles each; d_flows[p] is the field from frame p to
 * frame p + 1, bit for bit rsdsfm_deep_flow_dev(d_frames[p], d_frames[p + 1]).  Enqueued on the context's stream; returns without
 * waiting.  nframes >= 2, no NULL pointer in either array; rows, cols in [2, 16384]; channels 1 or 3; params NULL = defaults. */
int rsdsfm_deep_flow_seq_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                             const rsdsfm_flow_params* params_or_null, double* const* d_flows);

/* camera.cc:253-277 per consecutive pair (main.cc:380-457) on host buffers (same layouts); synchronous.  Staged one batch at a
 * time: the staging buffer holds B + 1 frames and B fields, never the whole clip. */
int rsdsfm_deep_flow_seq(rsdsfm_ctx* ctx, const uint8_t* const* frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                         const rsdsfm_flow_params* params_or_null, double* const* flows);

/* camera.cc:253-277, main.cc:380-457: pairs per batch of the two calls above and of rsdsfm_solve_video_dev: 1 .. 32, 0 = the
 * default (8).  Changes no result.  It sets the size of the context's sequence workspace (separate from rsdsfm_deep_flow_dev's):
 * about 120 bytes per pixel per pair (30 planes of the refinement) + 41 bytes per pixel per frame (B + 1 pyramids), i.e.
 * (120 B + 41 (B + 1)) bytes per pixel -- 1.2 GB at 1280x720 and 11 GB at 3840x2160 with B = 8; rebuilt when the size, the
 * pyramid parameters or B change, released by rsdsfm_destroy. */
int rsdsfm_set_flow_batch(rsdsfm_ctx* ctx, int32_t pairs);

/* camera.cc:253-277 + main.cc:380-457 for a whole clip: the flow of each batch of pairs on the context's stream, then
 * rsdsfm_solve_frames_dev over that batch's pairs (its lanes order themselves behind the context's stream).  results[p] is exactly
 * what rsdsfm_solve_frames_dev returns for the field of pair p with seed seeds[p] (seeds NULL: params->seed for every pair), with
 * d_depth_maps[p] and the pose tables d_R_or_null[p] / d_t_or_null[p] (either array may be NULL).  d_flows_or_null: where the
 * fields go (nframes - 1 device buffers); NULL = a library-owned ring of B buffers, reused batch after batch (safe:
 * rsdsfm_solve_frames_dev drains before it returns).  The device pointers inside results follow rsdsfm_solve_frames_dev's rule:
 * valid for the last `lanes` pairs of the last batch only; those of earlier batches are set to NULL.  Errors as
 * rsdsfm_solve_frames_dev reports them (the first one, "pair i: ..." numbered within the clip).  RSDSFM_ERR_INVALID for
 * nframes < 2, a NULL pointer inside an array, channels other than 1 or 3, a side outside [2, 16384], bad flow parameters. */
int rsdsfm_solve_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels, double fx,
                           double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                           const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows_or_null, double* const* d_depth_maps,
                           double* const* d_R_or_null, double* const* d_t_or_null, rsdsfm_frame_result* results);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_VIDEO_H */
