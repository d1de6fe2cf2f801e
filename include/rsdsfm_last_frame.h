/*
 * rsdsfm_last_frame.h -- C ABI of the clip's last frame on the MI355X: the last pair's depth map moved onto the last frame's own grid, and
 * that frame's pose table, so that a stabilised clip of F frames can have F frames.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  A
 * clip of F frames has F - 1 pairs, and every stage behind the solve renders frame p from PAIR p's depth map and pose table: the last frame
 * has no pair.  Nothing new has to be measured for it:
 *   - the flow model holds a pair's motion (v, w, k) constant over both of its frames, so pair F - 2's motion is the motion under which
 *     frame F - 1's scanlines were exposed;
 *   - the link and the fusion already move a pair's depths to its second capture (tests/link_spec_numpy.py: predict;
 *     tests/fuse_spec_numpy.py: splat_plane).  With a ratio of exactly 1.0 that splat IS the pair's depth map as a depth map of the second
 *     frame, in the pair's own unit;
 *   - the chain (rsdsfm_chain_clip) already gives A and c for all F frames.
 * tests/last_frame_spec_numpy.py is the executable definition; rsdsfm_advance_depth_dev reproduces it bit for bit, and
 * rsdsfm_last_frame_motion to rounding.  DESIGN.md section 12 ("Last frame") has the launches, the bytes and what has been measured.
 *
 * The clip calls take the frame through `last_frame` of rsdsfm_stabilize_params (rsdsfm_stabilize.h).
 *
 * NOT here: a depth for the pixels of the last frame that no pixel of the pair lands on (they stay 0 and the dense rectifier's depth fill
 * treats them like any hole), an occlusion test other than "the nearest surface wins", a motion of the last frame other than its pair's.
 */
#ifndef RSDSFM_LAST_FRAME_H
#define RSDSFM_LAST_FRAME_H

#include "rsdsfm_stabilize.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A pair's depth map moved to its second capture, as a depth map of the second frame.  d_field: the field the pair was solved on (rows x
 * cols x 2 doubles, row-major); d_depth_colmajor: the pair's depth map (rows x cols doubles, column-major, 0 where unknown); v3 / w3 / k:
 * the pair's final motion (HOST, read before the call returns); fx .. global_shutter: as rsdsfm_link_pairs_dev's.  Every pixel with a valid
 * depth (finite, > 0) and a usable vector (finite, not (0, 0)) whose landing pixel is inside offers its predicted depth z_pred (steps 1 - 4
 * of the link) to that pixel when z_pred is valid; among the offers to one pixel the smallest wins.
 *   d_depth_out_colmajor  rows x cols doubles, column-major: the winner, +0.0 where nothing landed
 *   d_plane_or_null       rows x cols uint64, row-major: the winners' bit patterns, all ones where nothing landed.  NULL: a plane of the
 *                         context's workspace (8 B per pixel, made on first use, released by rsdsfm_destroy)
 *   d_count_or_null       a DEVICE int64, 8-byte aligned: the number of pixels that received a value
 * Integer atomics only (a 64-bit unsigned minimum on the bit pattern -- positive finite doubles order as integers --, one 64-bit add per
 * workgroup for the count): the result is exact and does not depend on scheduling.  Enqueued on the context's stream; returns without
 * waiting.  RSDSFM_ERR_INVALID, with nothing written: a side outside [2, 16384], a NULL required pointer, an output that is an input or
 * another output, a field or plane that is not 16-byte aligned (the device API's rule), a counter that is not 8-byte aligned, a motion value
 * or gamma that is not finite, gamma <= 0, fx or fy not finite or 0, cx or cy not finite. */
int rsdsfm_advance_depth_dev(rsdsfm_ctx* ctx, const double* d_field, const double* d_depth_colmajor, const double v3[3], const double w3[3], double k,
                             int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double gamma, int32_t global_shutter,
                             double* d_depth_out_colmajor, uint64_t* d_plane_or_null, int64_t* d_count_or_null);

/* Kernel launches rsdsfm_advance_depth_dev enqueues for a rows x cols map: 3 (the plane's preset, the splat, the resolve; the counter is
 * zeroed by the splat).  RSDSFM_ERR_INVALID for a size outside [2, 16384].  Host only. */
int rsdsfm_advance_depth_launches(int32_t rows, int32_t cols);

/* The motion that puts the SECOND frame's scanlines into rsdsfm_pose_table_dev's form.  HOST arithmetic in double, no GPU, no context.
 * The table's law is beta_1(tau) = (tau + k tau^2 / 2) 2 / (2 + k) with tau = gamma i / rows; the second frame starts at tau = 1, and
 *   beta_1(1 + s) - beta_1(1) = (1 + k) (s + k' s^2 / 2) 2 / (2 + k),   k' = k / (1 + k),
 * which is the table's law for (v', w', k') with
 *   v' = v (2 + 3 k) / (2 + k),   w' = w (2 + 3 k) / (2 + k),   k' = k / (1 + k).
 * With k = 0 the factor is exactly 1 and the outputs are the inputs bit for bit.  The outputs may be the inputs.
 * RSDSFM_ERR_INVALID: a NULL pointer, a value that is not finite, 1 + k <= 0. */
int rsdsfm_last_frame_motion(const double v3[3], const double w3[3], double k, double v_out3[3], double w_out3[3], double* k_out);

/* The last frame's depth map and pose table from the last pair: byte for byte these public calls made one after another, enqueue only:
 *   1  rsdsfm_advance_depth_dev with these arguments into d_depth_out_colmajor (and the optional plane and counter);
 *   2  rsdsfm_last_frame_motion of (v3, w3, k);
 *   3  rsdsfm_pose_table_dev(ctx, v', w', k', gamma, rows, d_R_out, d_t_out) -- the call the clip solve makes for a pair's table, so that
 *      with k = 0 the last frame's table is its pair's own table byte for byte.
 * d_R_out: rows x 9, d_t_out: rows x 3 doubles.  Its errors are its parts'; nothing is enqueued when the motion is refused. */
int rsdsfm_last_frame_dev(rsdsfm_ctx* ctx, const double* d_field, const double* d_depth_colmajor, const double v3[3], const double w3[3], double k,
                          int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double gamma, int32_t global_shutter,
                          double* d_depth_out_colmajor, double* d_R_out, double* d_t_out, uint64_t* d_plane_or_null, int64_t* d_count_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_LAST_FRAME_H */
