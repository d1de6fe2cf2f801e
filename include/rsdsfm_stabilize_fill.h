/*
 * rsdsfm_stabilize_fill.h -- C ABI of the stabiliser's border fill on the MI355X: the band of a stabilised frame that its own frame does not
 * cover, filled from the neighbouring frames of the clip.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  The
 * stabiliser (rsdsfm_stabilize.h) neither zooms nor crops, so a stabilised frame has an empty band where the virtual camera sees what its own
 * frame does not, and the band moves from frame to frame.  Every frame's pose is in one coordinate system (rsdsfm_chain_clip), every pair
 * has a scale and a hole-free depth, and the stabiliser's map pass takes any rigid transform: frame n rendered into the virtual camera of
 * frame q is the stabiliser's stages A and B with
 *   M_{q,n} = A~_q^T A_n,   m_{q,n} = (A~_q^T (c_n - c~_q)) / S_n          (pair n's own unit)
 * -- a point X in the coordinates of frame n's first scanline is M X + m in virtual camera q's -- and a stage C that writes only where
 * the output is still empty.  The candidates of frame q are asked in the order n = q - 1, q + 1, q - 2, q + 2, ..., q - radius,
 * q + radius (nearer first, previous before next; only 0 <= n <= npairs - 1: the clip's last frame has no pair, hence no depth, unless
 * `last_frame` of rsdsfm_stabilize_params is set: rsdsfm_last_frame.h gives it the last pair's, and npairs then counts it); the first
 * that offers a pixel keeps it.  The SOURCE ID of the neighbour at offset j is 2 |j| for j < 0 and 2 |j| + 1 for j > 0; 1 is the own frame,
 * 0 nobody.
 * tests/stabilize_fill_spec_numpy.py is the executable definition; the frame call reproduces it bit for bit, the host function to rounding.
 * DESIGN.md section 12 ("Border fill") has the launches, the bytes and what has been measured.
 *
 * NOT here: blending or feathering at the seams, exposure compensation between frames, occlusion tests between candidates (a fold of a
 * neighbour's map fills like any pixel; built since: rsdsfm_stabilize_visible.h, asked for with `occlusion` below), moving objects,
 * inpainting of pixels nobody saw (built since: rsdsfm_stabilize_inpaint.h).  The clip's last frame is built since: rsdsfm_last_frame.h.
 */
#ifndef RSDSFM_STABILIZE_FILL_H
#define RSDSFM_STABILIZE_FILL_H

#include "rsdsfm_stabilize.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsdsfm_stabilize_fill_params {
    int32_t radius;       /* neighbours on each side, 1 .. 16; 0 = the default, 2, which is a choice, not a measurement */
    int32_t struct_bytes; /* 0 (zero-initialised struct) or sizeof(rsdsfm_stabilize_fill_params), as rsdsfm_stabilize_fill_params_init sets it;
                             anything else is refused: the caller was built against another layout */
    int32_t occlusion;    /* 0 = off: every byte of every clip call is what it was before the word had a name.  1 = the neighbour candidates
                             (source ids >= 2) of the clip calls go through rsdsfm_stabilize_visible_frame_dev (rsdsfm_stabilize_visible.h), in
                             the filled call with the window (0, 0, rows, cols).  Anything else is refused.  (The first of two words that were
                             `reserved`; the offset stays.) */
    int32_t occlusion_tol_q16; /* the test's tolerance in 1 / 65536: 0 = the default, 3277 (a choice, not a measurement), 1 .. 65536; anything
                             else is refused.  Read only when occlusion == 1.  (The second of the two words.) */
} rsdsfm_stabilize_fill_params;

/* radius = 2, struct_bytes = sizeof, occlusion = 0, occlusion_tol_q16 = 0 */
int rsdsfm_stabilize_fill_params_init(rsdsfm_stabilize_fill_params* params);

/* The candidates of frame q and their poses.  HOST arithmetic in double, no GPU, no context.  A / c: rsdsfm_chain_clip's, A_s / c_s:
 * rsdsfm_smooth_path's (entry q of the smoothed path and the listed neighbours' entries of the chain are read); scales: the chain's npairs
 * scales, ALWAYS read -- the baseline between two frames is real even when the path's translation is not smoothed (then c_s = c).
 * Writes *count_out <= 2 radius entries, in the order above: frames_out (the neighbour n), source_ids_out, M_out (x 9, row-major),
 * m_out (x 3); every array has room for 2 radius entries.  n = q is not listed: the own pose stays rsdsfm_virtual_poses'.
 * RSDSFM_ERR_INVALID: a NULL pointer, q outside [0, npairs - 1], radius outside [1, 16], a listed neighbour's scale that is not finite and
 * positive. */
int rsdsfm_neighbour_poses(const double* A, const double* c, const double* A_s, const double* c_s, const double* scales, int32_t npairs, int32_t q,
                           int32_t radius, int32_t* frames_out, int32_t* source_ids_out, double* M_out, double* m_out, int32_t* count_out);

/* One candidate: frame n (d_image_n, its depth map and pose table; rsdsfm_stabilize_frame_dev's arguments up to m3, its rules, its
 * errors) rendered into the virtual camera (M9, m3) and taken wherever d_mask_inout is 0 and the candidate is valid: there d_image_inout
 * gets the candidate's pixel -- the bytes rsdsfm_stabilize_frame_dev would write --, d_mask_inout 1 and d_source_or_null (rows x cols bytes)
 * source_id, 2 .. 255.  Nothing else is written; a candidate without one valid depth changes nothing.  d_mask_inout is REQUIRED.
 * d_filled_or_null: a DEVICE counter, 8-byte aligned: the number of pixels taken; the call zeroes it and the fill-warp kernel itself adds
 * to it (a sum per workgroup, one 64-bit integer atomic per workgroup: exact and independent of scheduling) -- no launch is added.
 * Image, mask and source plane must be 4-byte aligned; d_image_n may not be d_image_inout, the source plane may not be the mask.
 * Stages A and B run on the dense rectifier's workspace of the context: dense, stabilise and fill calls may alternate on one context
 * without a rebuild.  Enqueued on the context's stream; returns without waiting. */
int rsdsfm_stabilize_fill_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image_n, int32_t channels, const double* d_depth_n_colmajor, const double* d_R_n_rows9,
                                    const double* d_t_n_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int mode, int q5_mode,
                                    int32_t iterations, const double* M9, const double* m3, int32_t source_id, uint8_t* d_image_inout, uint8_t* d_mask_inout,
                                    uint8_t* d_source_or_null, int64_t* d_filled_or_null);

/* Kernel launches rsdsfm_stabilize_fill_frame_dev enqueues for a rows x cols frame: rsdsfm_rectify_dense_launches(rows, cols) -- the
 * fill-warp kernel stands where stage C stood and counts by itself.  The memset of the counter is not counted.  RSDSFM_ERR_INVALID for a
 * size outside [2, 16384].  Host only. */
int rsdsfm_stabilize_fill_launches(int32_t rows, int32_t cols);

/* A whole clip: rsdsfm_stabilize_video_dev (its arguments up to valid_or_null, its results, its rules, its errors; d_masks_out is REQUIRED
 * here), made unchanged, then for p = 0 .. nframes - 2 in order
 *   - the mask of frame p copied to d_sources_or_null[p] (rows x cols bytes; device to device), when passed: 1 = the own frame;
 *   - rsdsfm_neighbour_poses for q = p with fill_params_or_null's radius (NULL = the defaults);
 *   - one rsdsfm_stabilize_fill_frame_dev per listed neighbour n into d_stab_images[p], d_masks_out[p] and the source plane, with
 *     d_frames[n], pair n's FUSED map when d_fused_maps_or_null is passed (else its solved map), its pose table and mode / q5_mode /
 *     iterations as there.
 * Every output is, byte for byte, what those public calls give when made one after another; every output rsdsfm_stabilize_video_dev also
 * writes is what it writes alone, except the images and masks, and those differ only where the own mask was 0.
 * counts_or_null: HOST, (nframes - 1) x (2 + 2 radius) int64, per frame [none, own, offset -1, +1, -2, +2, ...] -- the index is the source
 * id; a skipped offset counts 0, none = rows cols - the rest, computed on the host.  With it the inner call is asked for its valid counts
 * (the `own` column; into valid_or_null or a buffer of this call's own) and waits as it does; the fill counts take one copy behind the last
 * launch and one wait.  Without it the fill passes are only enqueued on the context's stream.
 * With stabilize_params_or_null->last_frame == 1 the inner call renders the last frame too (see there), rsdsfm_neighbour_poses is asked with
 * nframes "pairs" and the loop runs p = 0 .. nframes - 1: the last frame has only previous candidates and is a candidate of the frames
 * before it, under the offsets' existing source ids.  d_masks_out, d_sources_or_null and counts_or_null then have nframes entries (rows),
 * like the inner call's per-frame arrays; the rule "byte for byte those public calls one after another" holds as it stands.
 * With fill_params_or_null->occlusion == 1 every candidate is one rsdsfm_stabilize_visible_frame_dev (rsdsfm_stabilize_visible.h) with the
 * window (0, 0, rows, cols) and occlusion_tol_q16 in the fill call's place, and the rule holds with that call named; the counts keep
 * their layout (the pixels taken), a rejected pixel shows up under a later offset or under `none`. */
int rsdsfm_stabilize_video_filled_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                      double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                      const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows, double* const* d_depth_maps,
                                      double* const* d_R, double* const* d_t, rsdsfm_frame_result* results,
                                      const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks_or_null,
                                      const rsdsfm_link_params* link_params_or_null, rsdsfm_link_record* records, double* scales, double* A, double* c,
                                      uint8_t* broken_or_null, const rsdsfm_fuse_params* fuse_params_or_null, double* const* d_fused_maps_or_null,
                                      const rsdsfm_stabilize_params* stabilize_params_or_null, int mode, int q5_mode, int32_t iterations, double* A_s,
                                      double* c_s, double* M, double* m, uint8_t* const* d_stab_images, uint8_t* const* d_masks_out,
                                      int64_t* valid_or_null, const rsdsfm_stabilize_fill_params* fill_params_or_null, uint8_t* const* d_sources_or_null,
                                      int64_t* counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_STABILIZE_FILL_H */
