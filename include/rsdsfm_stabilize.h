/*
 * rsdsfm_stabilize.h -- C ABI of the stabiliser on the MI355X: a smoothed camera path from a clip's trajectory, and every frame rendered
 * from its virtual camera on that path.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  The
 * dense rectifier (rsdsfm_rectify_dense.h) moves a rolling-shutter frame to the pose of its own first scanline: that removes the wobble
 * inside a frame and keeps the shake between frames.  Here
 *   1  the chain's poses (rsdsfm_chain_clip: X_0 = A_q X_q + c_q) are smoothed by ONE tangent-space mean step about every frame's own
 *      pose with Gaussian weights g_j = exp(-j^2 / (2 sigma^2)), |j| <= r, frames outside the clip skipped:
 *        A~_q = A_q exp([sum_j g_j log(A_q^T A_{q+j}) / sum_j g_j]x),   c~_q = c_q + sum_j g_j (c_{q+j} - c_q) / sum_j g_j
 *      (log: the rotation vector; a relative rotation near pi inside one window is ill-conditioned and unsupported, not detected).  A camera
 *      that does not move keeps its path bit for bit.
 *   2  the VIRTUAL POSE of frame q:  M_q = A~_q^T A_q,  m_q = (A~_q^T (c_q - c~_q)) / S_q  in pair q's own unit -- a point X in the
 *      coordinates of frame q's first scanline is M_q X + m_q in the virtual camera's.
 *   3  the dense rectifier with that one more rigid transform inside its stage B: pv = M pg + m behind the chain's pg, then the projection.
 *      Stages A and C are the dense rectifier's, unchanged; with M = I, m = 0 every output has the dense call's bytes.
 * tests/stabilize_spec_numpy.py is the executable definition; the frame call reproduces it bit for bit, the host functions to rounding
 * (they call exp, sin, cos, atan2).  DESIGN.md section 12 ("Stabilisation") has the launches, the bytes and what has been measured.
 *
 * There is NO zoom or crop parameter HERE: with a zoom folded into the displacement plane the fixed point p <- g - D(p) of stage C contracts
 * by |zoom - 1| per step and does not converge at zoom 2.  rsdsfm_stabilize_crop.h crops and zooms with D as it is and the target moved.
 */
#ifndef RSDSFM_STABILIZE_H
#define RSDSFM_STABILIZE_H

#include "rsdsfm_fuse.h"
#include "rsdsfm_rectify_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsdsfm_stabilize_params {
    double sigma;         /* the Gaussian's width in FRAMES; finite, > 0.  The default, 4.0, is a choice, not a measurement */
    int32_t radius;       /* the window's half width r in frames, 1 .. 1024; 0 = ceil(3 sigma) */
    int32_t translation;  /* 0: only the rotation is smoothed (c~ = c, m = 0; scales are not read) */
    int32_t struct_bytes; /* 0 (zero-initialised struct) or sizeof(rsdsfm_stabilize_params), as rsdsfm_stabilize_params_init sets it; anything
                             else is refused: the caller was built against another layout */
    int32_t last_frame;   /* 0: a clip call renders frames 0 .. nframes - 2, one per pair; 1: it also renders the clip's last frame from the last
                             pair's depth map moved onto that frame (rsdsfm_last_frame.h).  Anything else is refused.  (The word was
                             `reserved`, 0, before: same offset, same struct_bytes) */
} rsdsfm_stabilize_params;

/* sigma = 4.0, radius = 0, translation = 1, struct_bytes = sizeof */
int rsdsfm_stabilize_params_init(rsdsfm_stabilize_params* params);

/* Step 1.  HOST arithmetic in double, no GPU, no context.  A: nframes x 9 (row-major), c: nframes x 3 (rsdsfm_chain_clip's);
 * A_s / c_s: the smoothed path, same shapes (they may not overlap the inputs).  params_or_null: NULL = the defaults.  nframes >= 1.
 * RSDSFM_ERR_INVALID: a NULL pointer, nframes < 1, sigma not finite or <= 0, radius outside [0, 1024], bad struct_bytes. */
int rsdsfm_smooth_path(const double* A, const double* c, int32_t nframes, const rsdsfm_stabilize_params* params_or_null, double* A_s, double* c_s);

/* Step 2.  HOST.  A / c / A_s / c_s: entries 0 .. npairs - 1 are read; scales: rsdsfm_chain_clip's npairs scales (not read, and may be
 * NULL, when translation == 0).  M: npairs x 9, m: npairs x 3.  npairs >= 1.  RSDSFM_ERR_INVALID: a NULL pointer, npairs < 1, a scale
 * that is not finite and positive. */
int rsdsfm_virtual_poses(const double* A, const double* c, const double* A_s, const double* c_s, const double* scales, int32_t npairs,
                         int32_t translation, double* M, double* m);

/* Step 3, one frame: rsdsfm_rectify_dense_frame_dev (its arguments up to `iterations`, its outputs, its rules, its errors) seen from the
 * virtual camera M9 (row-major) / m3 -- HOST pointers, read before the call returns; RSDSFM_ERR_INVALID when either is NULL or holds a value
 * that is not finite.  d_valid_or_null: a DEVICE counter, 8-byte aligned: the number of mask pixels that are 1; the call zeroes it and one
 * more launch sets it (the mask is read as 32-bit words with a byte tail, one 64-bit integer atomic per workgroup: exact and independent of
 * scheduling).  A count without d_mask_or_null takes a mask plane of the context's workspace (1 B per pixel, made when first asked for).
 * The pyramid and the displacement plane are the dense rectifier's workspace of the context: dense and stabilise calls may alternate on one
 * context without a rebuild.  Enqueued on the context's stream; returns without waiting. */
int rsdsfm_stabilize_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, int32_t channels, const double* d_depth_map_colmajor, const double* d_R_rows9,
                               const double* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int mode, int q5_mode,
                               int32_t iterations, const double* M9, const double* m3, uint8_t* d_image_out, uint8_t* d_mask_or_null,
                               double* d_filled_depth_or_null, float* d_disp_or_null, int64_t* d_valid_or_null);

/* Kernel launches rsdsfm_stabilize_frame_dev enqueues for a rows x cols frame: rsdsfm_rectify_dense_launches(rows, cols) -- the stabiliser's
 * map kernel stands where the dense one stood --, plus one when count != 0 (d_valid_or_null is passed).  The memset of the counter and the
 * copy of d_disp_or_null are not counted.  RSDSFM_ERR_INVALID for a size outside [2, 16384].  Host only. */
int rsdsfm_stabilize_launches(int32_t rows, int32_t cols, int32_t count);

/* A whole clip: rsdsfm_solve_video_linked_dev (its arguments up to broken_or_null, its results, its rules, its errors) with d_flows,
 * d_depth_maps, d_R and d_t all REQUIRED (every pair's pose table must outlive the solve, and the lanes' scratch tables do not), then
 *   - when d_fused_maps_or_null is passed (nframes - 1 buffers of rows x cols doubles): rsdsfm_fuse_depths_dev with fuse_params_or_null on
 *     the call's own fields, maps, motions and records; the renderer then reads the FUSED maps, else the solve's;
 *   - rsdsfm_smooth_path with stabilize_params_or_null and rsdsfm_virtual_poses on the chain: A_s (nframes x 9), c_s (nframes x 3),
 *     M ((nframes - 1) x 9), m ((nframes - 1) x 3), all HOST;
 *   - for p = 0 .. nframes - 2 in order, rsdsfm_stabilize_frame_dev of d_frames[p] with pair p's map and pose table and (M_p, m_p) into
 *     d_stab_images[p] (rows x cols x channels bytes) and d_masks_out_or_null[p] (rows x cols bytes), mode / q5_mode / iterations as there.
 * The smoothing is not causal, so nothing hooks into the solve.  Every output is, byte for byte, what those public calls give when made one
 * after another.  The last frame has no pair and is not rendered unless `last_frame` is set.  A broken link carries its scale over, as in the
 * chain; with translation == 0 the scales are not read at all.  valid_or_null: nframes - 1 HOST counts, fetched in one copy behind the last
 * frame, which the call then waits for; without it the frames are only enqueued on the context's stream.
 *
 * With stabilize_params_or_null->last_frame == 1 (np = nframes - 1), behind the solve, the wait for its lanes and the fusion:
 *   - rsdsfm_last_frame_dev (rsdsfm_last_frame.h) on pair np - 1's field, solved map and final motion into d_depth_maps[np], d_R[np], d_t[np];
 *   - when fused maps are requested, rsdsfm_advance_depth_dev of d_fused_maps[np - 1] with the same field and motion into d_fused_maps[np];
 *   - scales[np] = scales[np - 1];
 *   - rsdsfm_virtual_poses with np + 1, and the frame loop runs p = 0 .. np.
 * Then d_depth_maps, d_R, d_t, d_fused_maps_or_null, scales, M, m, d_stab_images, d_masks_out_or_null and valid_or_null have nframes
 * entries; results, d_flows, seeds, d_masks_or_null, records and broken keep nframes - 1 (nframes - 2 for the links).  Every output is still,
 * byte for byte, what those public calls give when made one after another, and everything the solve writes is what it writes without the
 * flag. */
int rsdsfm_stabilize_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                               double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                               const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows, double* const* d_depth_maps,
                               double* const* d_R, double* const* d_t, rsdsfm_frame_result* results,
                               const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks_or_null,
                               const rsdsfm_link_params* link_params_or_null, rsdsfm_link_record* records, double* scales, double* A, double* c,
                               uint8_t* broken_or_null, const rsdsfm_fuse_params* fuse_params_or_null, double* const* d_fused_maps_or_null,
                               const rsdsfm_stabilize_params* stabilize_params_or_null, int mode, int q5_mode, int32_t iterations, double* A_s,
                               double* c_s, double* M, double* m, uint8_t* const* d_stab_images, uint8_t* const* d_masks_out_or_null,
                               int64_t* valid_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_STABILIZE_H */
