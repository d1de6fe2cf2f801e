/*
 * rsdsfm_trajectory.h -- C ABI of a clip's trajectory on the MI355X: the relative scale of consecutive pairs, the camera's pose at every
 * frame, and the clip's world points in one coordinate system.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to any of
 * this: a differential solve fixes its scale per pair, so pair p's v and depth map are in one arbitrary unit and pair p + 1's in another.
 * The LINK between the two measures the ratio of the units from the pixels both pairs gave a depth to: pair p's depth at a pixel, moved
 * to the second capture by pair p's own motion under the model the solve fits, against pair p + 1's depth where pair p's flow lands.
 * tests/link_spec_numpy.py is the executable definition, operation by operation, in float64; the kernels (csrc/link_kernels.hip)
 * reproduce the link and the points bit for bit.  DESIGN.md section 12 ("Trajectory") has the bytes per pixel, the launches, the
 * workspace and what has been measured.
 *
 * The time base is the FLOW MODEL's, u = beta (A v rho + B w) with u = flow * gamma / f (minimal.cc:257-266): between the two captures of
 * a point, (v, w) acts for b = beta / gamma; from scanline 0 of one frame to scanline 0 of the next, for 1 / gamma.
 * RsFrame::setRelativePose's table (rsdsfm_pose_table_dev) moves scanline i by gamma * i / rows * v, a factor gamma from what the flow
 * model implies; the pose tables and the rectifiers keep the reference's convention, the link and the trajectory follow the solve's.
 *
 * The per-pair pose tables keep the reference's first-order rotation I + [w]x.  The chain uses the exact exponential (Rodrigues): a
 * product of F - 1 matrices that are not orthonormal drifts, and a trajectory is what gets plotted.
 */
#ifndef RSDSFM_TRAJECTORY_H
#define RSDSFM_TRAJECTORY_H

#include "rsdsfm_flow_check.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsdsfm_link_params {
    double tol;           /* a correspondence AGREES with the median iff r <= ratio (1 + tol) and r (1 + tol) >= ratio; finite, >= 0 (0.1) */
    int32_t min_links;    /* a link with fewer correspondences is not valid; >= 0 (16) */
    int32_t radix_bits;   /* digit width of the selection: 0 = the default (11: six passes), 8 (eight passes) or 11.  Which launches run,
                             never a result */
    int32_t struct_bytes; /* 0 (zero-initialised struct) or sizeof(rsdsfm_link_params), as rsdsfm_link_params_init sets it; anything else is
                             refused: the caller was built against another layout */
    int32_t reserved;     /* 0 */
} rsdsfm_link_params;

/* tol = 0.1, min_links = 16, radix_bits = 0, struct_bytes = sizeof */
int rsdsfm_link_params_init(rsdsfm_link_params* params);

typedef struct rsdsfm_link_record {
    int64_t n;      /* correspondences */
    double ratio;   /* their lower median (rank (n - 1) / 2 in sorted order: one of them, exactly); NaN when n = 0 */
    int64_t agree;  /* correspondences within tol of the median */
    int32_t valid;  /* n >= min_links */
    int32_t reserved;
} rsdsfm_link_record;

/* The links of a clip's solved pairs (main.cc:380-457 per pair; rsdsfm_solve_video_dev's outputs), composed of the ratio pass, the radix
 * selection and the agree pass of csrc/link_kernels.hip.  npairs >= 2 pairs give npairs - 1 links; link p reads d_fields[p] (the field
 * pair p was solved on, rows x cols x 2 doubles, row-major; a masked field of the checked calls is fine; d_fields[npairs - 1] is not read
 * and may be NULL), d_depth_maps[p] and d_depth_maps[p + 1] (rows x cols doubles, column-major: the solve's maps, inlier depths only), and
 * pair p's final motion v_3n[3 p ..], w_3n[3 p ..], k_n[p] (HOST arrays; after refinement and sign canonicalisation).  global_shutter:
 * whether the solve ran with use_global_shutter_mode (alpha = 1).  d_ratio_planes_or_null: npairs - 1 device buffers of rows x cols
 * uint64 (row-major) that receive each link's plane -- the ratio's bit pattern, 0 = no correspondence; NULL = planes of the context's
 * workspace (8 bytes per pixel per link, at most 32 links in flight; made on first use, released by rsdsfm_destroy).  records: npairs - 1
 * HOST records.  All links of a call (of each 32) run in the same launches: 2 + 2 ceil(64 / radix_bits) of them, without a host wait in
 * between; the scalars come back in ONE copy behind the last launch, which the call waits for.  Exact and independent of scheduling:
 * integer atomics only.  RSDSFM_ERR_INVALID: npairs < 2, a side outside [2, 16384], a NULL required pointer, a plane that is an input, bad
 * parameters (tol negative or not finite, min_links < 0, radix_bits not 0 / 8 / 11, struct_bytes). */
int rsdsfm_link_pairs_dev(rsdsfm_ctx* ctx, const double* const* d_fields, const double* const* d_depth_maps, const double* v_3n, const double* w_3n,
                          const double* k_n, int32_t npairs, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double gamma,
                          int32_t global_shutter, const rsdsfm_link_params* params_or_null, uint64_t* const* d_ratio_planes_or_null,
                          rsdsfm_link_record* records);

/* The chain: HOST arithmetic in double, no GPU, no context (main.cc:380-523 solves the pairs one by one and never relates them).
 * records: the npairs - 1 links; v_3n / w_3n: the pairs' motions.  Outputs (F = npairs + 1 frames):
 *   scales[npairs]      S_0 = 1, S_{q+1} = S_q / ratio_q; where link q is not valid (or its ratio is not a positive finite number)
 *                       S_{q+1} = S_q and broken_or_null[q] = 1.  Pair q's depths and translation in clip units are S_q Z_q and S_q v_q.
 *   A[F][9], c[F][3]    frame q's first scanline in frame 0's coordinates (X_0 = A_q X_q + c_q; row-major):  A_0 = I, c_0 = 0,
 *                       R_q = exp([w_q / gamma]x) (Rodrigues, exact: see the head of this file), A_{q+1} = A_q R_q^T,
 *                       c_{q+1} = c_q - A_{q+1} (S_q v_q / gamma).
 *   broken_or_null[npairs - 1]
 * npairs >= 1 (one pair: no link, records may be NULL).  RSDSFM_ERR_INVALID for a NULL pointer, npairs < 1, gamma not finite or <= 0. */
int rsdsfm_chain_clip(const rsdsfm_link_record* records, const double* v_3n, const double* w_3n, int32_t npairs, double gamma, double* scales, double* A,
                      double* c, uint8_t* broken_or_null);

/* The clip's points (main.cc:480-523 writes each pair's world points in that pair's own frame and unit): d_points_in[q], q < npairs, are
 * pair q's world points, rows x cols x 3 floats in frame q's coordinates (rsdsfm_rectify_frame_dev's d_coords3d); d_points_out[q] receives
 * A_q (S_q X) + c_q, computed in float64 and rounded once to float.  d_points_out[q] may equal d_points_in[q] (in place); no other overlap.
 * A point that is exactly (0, 0, 0) stays (0, 0, 0): that is what the rectifier writes for a pixel it skips.  (A pixel without depth
 * carries its scanline's camera centre there, which is (0, 0, 0) on scanline 0 only; it is transformed like any point and lands on that
 * centre in clip coordinates.  Select points by the depth map.)  scales / A / c: rsdsfm_chain_clip's (HOST; entries 0 .. npairs - 1 are
 * read).  One streaming launch per 16 pairs, enqueued on the context's stream; returns without waiting. */
int rsdsfm_clip_points_dev(rsdsfm_ctx* ctx, const float* const* d_points_in, float* const* d_points_out, int32_t npairs, int32_t rows, int32_t cols,
                           const double* scales, const double* A, const double* c);

/* rsdsfm_solve_video_dev (its arguments up to `results`, its rules, its errors) -- or, when d_masks_or_null is passed,
 * rsdsfm_solve_video_checked_dev with check_params_or_null and those masks -- and then rsdsfm_link_pairs_dev on its outputs,
 * rsdsfm_chain_clip and, when d_points_or_null is passed, rsdsfm_clip_points_dev in place.  Nothing is added inside the solve: every
 * per-pair result, field, depth map and pose table is that call's, bit for bit, and the records, scales and poses are what the three calls
 * above give on them.  d_flows is REQUIRED here (RSDSFM_ERR_INVALID for NULL): the library's ring keeps only B fields, and link p reads
 * pair p's field after pair p + 1 has been solved.  records: nframes - 2; scales: nframes - 1; A: nframes x 9; c: nframes x 3;
 * broken_or_null: nframes - 2 (all HOST).  d_points_or_null: nframes - 1 device buffers that hold each pair's world points in its own
 * frame when the call is made (e.g. rsdsfm_rectify_video_dev's d_coords3d of the same clip, parameters and seeds) and the clip's when it
 * returns.  Synchronous in the records and poses; the points are enqueued on the context's stream. */
int rsdsfm_solve_video_linked_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                  double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                  const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows, double* const* d_depth_maps,
                                  double* const* d_R_or_null, double* const* d_t_or_null, rsdsfm_frame_result* results,
                                  const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks_or_null,
                                  const rsdsfm_link_params* link_params_or_null, rsdsfm_link_record* records, double* scales, double* A, double* c,
                                  uint8_t* broken_or_null, float* const* d_points_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_TRAJECTORY_H */
