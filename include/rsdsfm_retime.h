/*
 * rsdsfm_retime.h -- C ABI of the retimer on the MI355X: a frame of a solved clip rendered at ANY instant along the camera path, from the two
 * input frames next to it in time.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  A
 * stabilised clip (rsdsfm_stabilize.h and the headers behind it) has one output frame per input frame, at the input's own instants.  With the
 * chain's poses (rsdsfm_chain_clip), a scale and a hole-free depth per pair and a map pass that takes any rigid transform, a static scene can
 * be rendered at a time BETWEEN two frames: frame-rate conversion, slow motion, constant pacing from irregular input.
 *   path        the pose at time t, q = floor(t), tau = t - q: entry q itself when tau == 0, else
 *               A_t = A_q exp([tau so3_log(A_q^T A_{q+1})]x), c_t = c_q + tau (c_{q+1} - c_q) -- piecewise geodesic, rsdsfm_smooth_path's
 *               logarithm and exponential.
 *   sources     n0 = floor(t) and, when tau > 0, n1 = n0 + 1; for each M = A_t^T A_n, m = A_t^T (c_n - c_t) / S_n (rsdsfm_neighbour_poses'
 *               expressions): a point X in frame n's first-scanline coordinates is M X + m in the camera at t.
 *               weight w = 0 with one source, else rint(tau 65536) clamped to [1, 65535], in 1 / 65536.
 *   layers      every source rendered ALONE onto a zeroed layer (rsdsfm_stabilize_window_frame_dev, or through the occlusion test:
 *               rsdsfm_stabilize_visible_frame_dev / rsdsfm_stabilize_search_frame_dev), layer A from n0 and layer B from n1.
 *   merge       per pixel, a = mask_a != 0, b = mask_b != 0, d = max over the channels of |a_c - b_c|:
 *               neither                          image 0, mask 0, source 0
 *               a only                           a's bytes, mask 1, source 1 (RSDSFM_RETIME_FROM_A)
 *               b only                           b's bytes, mask 1, source 2 (RSDSFM_RETIME_FROM_B)
 *               both, d <= threshold             out_c = (a_c (65536 - w) + b_c w + 32768) >> 16, mask 1, source 3 (dissolved)
 *               both, d > threshold, w <= 32768  a's bytes, mask 1, source 4  (the views disagree -- misregistration, a moving object, a
 *               both, d > threshold, w > 32768   b's bytes, mask 1, source 5   fold --: the source nearer in time is taken)
 * Integers only in the merge; tests/retime_spec_numpy.py is the executable definition and every call here reproduces it bit for bit.
 * DESIGN.md section 12 ("Retime") has the kernel, the launches, the bytes and what has been measured.
 *
 * NOT here: splines through the poses (the path is piecewise geodesic), filling from further neighbours and inpainting (the generic frame
 * calls rsdsfm_stabilize_window_frame_dev, rsdsfm_seam_blend_layer_dev and rsdsfm_inpaint_frame_dev accept this header's outputs), an
 * exposure gain between the two sources, a fused two-source warp that skips the layers, the C++ mirror.
 */
#ifndef RSDSFM_RETIME_H
#define RSDSFM_RETIME_H

#include "rsdsfm_stabilize_search.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the merge's source plane */
#define RSDSFM_RETIME_NONE 0
#define RSDSFM_RETIME_FROM_A 1
#define RSDSFM_RETIME_FROM_B 2
#define RSDSFM_RETIME_DISSOLVED 3
#define RSDSFM_RETIME_CONFLICT_A 4
#define RSDSFM_RETIME_CONFLICT_B 5
#define RSDSFM_RETIME_THRESHOLD_DEFAULT 24 /* a choice, not a measurement */

typedef struct rsdsfm_retime_params {
    int32_t threshold;         /* 0 .. 255, taken as it stands (0 is a threshold, not "the default"); 255: the plain cross-dissolve */
    int32_t occlusion;         /* 0: the layers through rsdsfm_stabilize_window_frame_dev; 1: through the occlusion test */
    int32_t occlusion_tol_q16; /* the occlusion test's tolerance, 1 .. 65536; 0: its default */
    int32_t struct_bytes;      /* 0 or sizeof(rsdsfm_retime_params), as rsdsfm_retime_params_init sets it; anything else is refused */
    int32_t reserved[4];       /* 0 */
} rsdsfm_retime_params;

/* threshold = 24, occlusion = 0, occlusion_tol_q16 = 0, struct_bytes = sizeof.  A NULL params pointer means these values. */
int rsdsfm_retime_params_init(rsdsfm_retime_params* params);

/* HOST only, double, no context: the pose at time t on a path of nposes poses (A_path: nposes x 9 row-major, c_path: nposes x 3), as defined
 * above, into A_t9 and c_t3.  An integer t returns the entry's bytes.
 * RSDSFM_ERR_INVALID: a NULL pointer, nposes < 1, t not finite or outside [0, nposes - 1]. */
int rsdsfm_path_at(const double* A_path, const double* c_path, int32_t nposes, double t, double* A_t9, double* c_t3);

/* HOST only: the sources of the frame at time t and their poses.  A, c: the chain's poses; A_path, c_path: the path to ride (the smoothed
 * path, or the chain itself); scales: one per source; nsources: the frames that have a depth map and a pose table (the clip's pairs, or its
 * frames after a last_frame clip call); t in [0, nsources - 1].  src_out[0] = floor(t), src_out[1] = src_out[0] + 1 or -1; *nsrc_out 1 or 2;
 * *weight_q16_out as above; M_out (2 x 9) and m_out (2 x 3) get an entry per source (the second untouched with one source); A_t9, c_t3: the
 * pose at t (rsdsfm_path_at over the first nsources poses).  At an integer t, (M, m) are rsdsfm_virtual_poses' entry for that path.
 * RSDSFM_ERR_INVALID: a NULL pointer, nsources < 1, t not finite or out of range, a listed source's scale not finite and positive. */
int rsdsfm_retime_poses(const double* A, const double* c, const double* A_path, const double* c_path, const double* scales, int32_t nsources, double t,
                        int32_t src_out[2], int32_t* nsrc_out, int32_t* weight_q16_out, double* M_out, double* m_out, double* A_t9, double* c_t3);

/* The merge of two layers (image: rows x cols x channels bytes, channels 1 or 3; mask: rows x cols bytes, 0 = empty, anything else set; all
 * DEVICE, only read) into d_image_out, d_mask_out and d_source_or_null as defined above: every byte of the output planes is written, so they
 * need no preset.  d_image_b_or_null and d_mask_b_or_null both NULL: b is absent everywhere, and weight_q16 must be 0.  weight_q16 0 .. 65535,
 * threshold 0 .. 255, rows and cols in [2, 16384].
 * d_counts5_or_null: a DEVICE array [none, a only, b only, dissolved, conflict] of five int64, 8-byte aligned; the call zeroes it (a memset on
 * the context's stream) and the kernel adds to it -- a sum per workgroup with shuffles and LDS, then five 64-bit integer atomics per workgroup:
 * exact and independent of scheduling.
 * Every plane is 4-byte aligned; the outputs are distinct from the inputs and from each other.  One kernel launch, enqueued on the context's
 * stream; returns without waiting.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased pointer, only one of the two b pointers, channels, a size, weight_q16 or threshold outside
 * its range, a weight other than 0 without b. */
int rsdsfm_retime_merge_dev(rsdsfm_ctx* ctx, const uint8_t* d_image_a, const uint8_t* d_mask_a, const uint8_t* d_image_b_or_null, const uint8_t* d_mask_b_or_null,
                            int32_t channels, int32_t rows, int32_t cols, int32_t weight_q16, int32_t threshold, uint8_t* d_image_out, uint8_t* d_mask_out,
                            uint8_t* d_source_or_null, int64_t* d_counts5_or_null);

/* Kernel launches of rsdsfm_retime_merge_dev: 1.  The memset of the counters is not counted.  Host only. */
int rsdsfm_retime_merge_launches(void);

/* One frame at one instant.  d_images, d_depths_colmajor, d_R_rows9, d_t_rows3: HOST arrays of nsrc DEVICE pointers, a source's image
 * (rows x cols x channels bytes), depth map (column-major doubles, 0 where unknown) and pose table, as rsdsfm_stabilize_window_frame_dev takes
 * them; the camera, rows, cols, mode, q5_mode and iterations are that call's.  nsrc 1 or 2; M18, m6, weight_q16: rsdsfm_retime_poses' (with one
 * source the weight must be 0 and the second entries are not read).  window_or_null: (r0, c0, h, w), NULL = the full frame.
 * In order, on the context's stream: layer A's image and mask zeroed, source 0 rendered alone onto layer A, with two sources the same for
 * layer B, then rsdsfm_retime_merge_dev (NULL b with one source) into the four outputs.  The render is rsdsfm_stabilize_window_frame_dev with
 * params->occlusion == 0; with 1 it is rsdsfm_stabilize_visible_frame_dev, or rsdsfm_stabilize_search_frame_dev when the context's
 * rsdsfm_set_occlusion_search knob is 1, with params->occlusion_tol_q16.  Every output is byte for byte what those public calls give when
 * made one after another.  Layer A is the blended clip's layer of the context's dense workspace; layer B joins the workspace when first asked
 * for and is released by rsdsfm_destroy: a context that never asks keeps its footprint.  Returns without waiting.
 * RSDSFM_ERR_INVALID: the merge's and the render calls' lists, nsrc, a weight other than 0 with one source, a NULL or non-finite M18 / m6,
 * occlusion other than 0 / 1, occlusion_tol_q16 outside [0, 65536], threshold outside [0, 255], bad struct_bytes. */
int rsdsfm_retime_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                            const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                            int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M18, const double* m6, int32_t weight_q16,
                            const rsdsfm_retime_params* params_or_null, const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out,
                            uint8_t* d_source_or_null, int64_t* d_counts5_or_null);

/* = nsrc rsdsfm_stabilize_window_launches(rows, cols) + 1.  RSDSFM_ERR_INVALID for a size outside [2, 16384] or nsrc other than 1 / 2.  Host only. */
int rsdsfm_retime_launches(int32_t rows, int32_t cols, int32_t nsrc);

/* A clip, retimed AFTER it was solved: the call reads what rsdsfm_stabilize_video_dev or one of its variants left behind -- d_frames, the
 * nsources depth maps (solved or fused: the caller's choice), d_R, d_t (arrays of nsources DEVICE pointers) and the HOST arrays A, c, the path
 * A_path, c_path and scales -- and renders ntimes frames: for i = 0 .. ntimes - 1 in order rsdsfm_retime_poses(times[i]) and
 * rsdsfm_retime_frame_dev into d_out_images[i], d_out_masks[i], d_out_sources_or_null[i] (the array may be NULL).  Every plane and host array is
 * byte for byte what those calls give when made one after another.
 * sources_out: HOST, ntimes x 2 int32, -1 for an absent source.  weights_out: HOST, ntimes int32.  counts_or_null: HOST, ntimes x 5 int64, the
 * merge's counters; with it the call ends with one copy and one wait, without it the call only enqueues.
 * RSDSFM_ERR_INVALID: a NULL array or entry, ntimes < 1, a time rsdsfm_retime_poses refuses (nothing is enqueued then), and the frame call's list. */
int rsdsfm_retime_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                            double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                            const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                            const double* times, int32_t ntimes, const rsdsfm_retime_params* params_or_null, const int32_t* window_or_null,
                            uint8_t* const* d_out_images, uint8_t* const* d_out_masks, uint8_t* const* d_out_sources_or_null, int32_t* sources_out,
                            int32_t* weights_out, int64_t* counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_RETIME_H */
