/*
 * rsdsfm_stabilize_crop.h -- C ABI of the stabiliser's crop and zoom on the MI355X: ONE window for the whole clip, found on the GPU from the
 * masks the stabiliser already writes, and every frame rendered once through it at full size.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  The
 * stabiliser (rsdsfm_stabilize.h) and its border fill (rsdsfm_stabilize_fill.h) leave a band that moves from frame to frame and pixels
 * nobody saw.  A zoom folded into the displacement plane D makes stage C's fixed point p <- g - D(p) contract by |zoom - 1| and was never
 * built.  Here D stays as it is and the TARGET moves: output pixel g = (ix, iy) of the full-size frame is mapped into the window
 * (r0, c0, h, w),
 *   tx = (c0 + (ix + 0.5) (w / cols)) - 0.5,   ty = (r0 + (iy + 0.5) (h / rows)) - 0.5          (in that operation order)
 * and stage C solves p + D(p) = t by p = t, p <- t - D(p): the contraction is D's own, exactly as without a zoom.  The frame is rendered
 * once, directly at the zoomed positions, with one bilinear interpolation; it is not resampled from a rendered frame.  With the window
 * (0, 0, rows, cols) the targets are exactly the integers and every byte is the un-windowed call's.
 * The window is the same for the whole clip (a window per frame would put the shake back as zoom jitter): the largest rectangle of the
 * frame's aspect ratio, w(h) = (h cols) / rows floored, whose surroundings within `margin` pixels hold at most `max_empty` pixels that are
 * empty in ANY of the masks; ties go to the one nearest the frame's centre (the smallest |2 r0 + h - rows| + |2 c0 + w - cols|), then to the
 * smallest r0, then the smallest c0.  The horizontal and vertical scales differ because w is floored: less than one source pixel across the
 * frame.
 * A fitted window does NOT guarantee a full output mask: a target between two valid integer pixels can still leave the frame where the
 * filled depth is rough.  The counts say what happened.
 * tests/stabilize_crop_spec_numpy.py is the executable definition; every call here reproduces it bit for bit.  DESIGN.md section 12 ("Crop
 * and zoom") has the kernels, the launches, the bytes and what has been measured.
 *
 * NOT here: windows that vary over time, path optimisers that trade smoothness against crop, a search that re-renders until the mask is
 * full, blending at the seams.  The clip's last frame is built since: rsdsfm_last_frame.h.
 */
#ifndef RSDSFM_STABILIZE_CROP_H
#define RSDSFM_STABILIZE_CROP_H

#include "rsdsfm_stabilize_fill.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsdsfm_stabilize_crop_params {
    int64_t max_empty;    /* empty pixels the window and its margin may hold, 0 .. rows cols; the default is 0 */
    int32_t margin;       /* pixels around the window that count as well, 0 .. 64 (the frame's own edge is not a hole).  The default, 1, is a
                             choice, not a measurement */
    int32_t struct_bytes; /* 0 (zero-initialised struct: max_empty 0, margin 0) or sizeof(rsdsfm_stabilize_crop_params), as
                             rsdsfm_stabilize_crop_params_init sets it; anything else is refused */
    int32_t reserved[4];  /* 0 */
} rsdsfm_stabilize_crop_params;

/* max_empty = 0, margin = 1, struct_bytes = sizeof */
int rsdsfm_stabilize_crop_params_init(rsdsfm_stabilize_crop_params* params);

/* The window of nmasks (1 .. 4096) DEVICE planes of rows x cols bytes (0 = empty, anything else set; 4-byte aligned; d_masks itself is a HOST
 * array of device pointers), rows and cols in [2, 16384]: window_out = (r0, c0, h, w), HOST; (0, 0, 0, 0) when nothing fits.
 * params_or_null: NULL = the defaults.  Three kernels on the context's stream -- the AND of the planes and the prefix count of its empties
 * along every row, the sums down the columns (a summed-area table of (rows + 1) x (cols + 1) uint32 in the context's dense workspace, made
 * when first asked for and released by rsdsfm_destroy), and the search: one anchor per lane, a binary search over the height with 4 table
 * loads per step, the result packed into one 64-bit key and reduced with one 64-bit integer atomicMax per workgroup: exact and independent
 * of scheduling.  The planes are only read.  The call WAITS for one 8-byte copy, the winning key, and decodes it on the host.
 * RSDSFM_ERR_INVALID: a NULL or misaligned pointer, nmasks, a size, margin or max_empty outside its range, bad struct_bytes. */
int rsdsfm_crop_window_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_masks, int32_t nmasks, int32_t rows, int32_t cols,
                           const rsdsfm_stabilize_crop_params* params_or_null, int32_t window_out[4]);

/* Kernel launches of rsdsfm_crop_window_dev: 3.  The memset of the key is not counted.  RSDSFM_ERR_INVALID for a size outside [2, 16384].
 * Host only. */
int rsdsfm_crop_window_launches(int32_t rows, int32_t cols);

/* One frame through a window: rsdsfm_stabilize_fill_frame_dev (its arguments, its rules, its errors) with the targets above in stage C's
 * fixed point; the output is rows x cols, full size.  source_id is 1 .. 255: 1 means the own frame, rendered onto a zeroed mask.  Pixels are
 * taken only where d_mask_inout is 0, and counted the same way (a sum per workgroup, one 64-bit integer atomicAdd).  window = (r0, c0, h, w),
 * HOST, read before the call returns; RSDSFM_ERR_INVALID when it is NULL, h < 1, w < 1, r0 < 0, c0 < 0, r0 + h > rows or c0 + w > cols.
 * With (0, 0, rows, cols) every byte is rsdsfm_stabilize_fill_frame_dev's.  Stages A and B are the existing launches, unchanged. */
int rsdsfm_stabilize_window_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image_n, int32_t channels, const double* d_depth_n_colmajor, const double* d_R_n_rows9,
                                      const double* d_t_n_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int mode, int q5_mode,
                                      int32_t iterations, const double* M9, const double* m3, int32_t source_id, const int32_t window[4], uint8_t* d_image_inout,
                                      uint8_t* d_mask_inout, uint8_t* d_source_or_null, int64_t* d_filled_or_null);

/* = rsdsfm_stabilize_fill_launches(rows, cols).  Host only. */
int rsdsfm_stabilize_window_launches(int32_t rows, int32_t cols);

/* A whole clip, cropped and zoomed: rsdsfm_stabilize_video_filled_dev (its arguments up to counts_or_null, its results, its rules, its
 * errors) made unchanged -- with a fill radius of 0 .. 16 here: at radius 0 (the struct's field; a NULL fill_params_or_null is the fill's
 * default, 2) the inner call is rsdsfm_stabilize_video_dev, d_sources_or_null is not written and counts_or_null gets [none, own] -- then
 *   - rsdsfm_crop_window_dev with crop_params_or_null on that call's nframes - 1 output masks (d_masks_out, REQUIRED), unless
 *     window_in_or_null (HOST, 4 values) is given: then the search is skipped and that window is used;
 *   - for p = 0 .. nframes - 2 in order: d_crop_masks[p] and d_crop_sources_or_null[p] zeroed, one rsdsfm_stabilize_window_frame_dev for the
 *     own frame (rsdsfm_virtual_poses' pose, id 1) and one per neighbour of rsdsfm_neighbour_poses, in its order, into d_crop_images[p]
 *     (rows x cols x channels bytes; zeroed first), d_crop_masks[p] and the source plane -- on the FUSED maps when d_fused_maps_or_null is
 *     passed.
 * Every output is byte for byte what those public calls give when made one after another; everything the inner call writes is what it
 * writes alone.  window_out: HOST, the window used.  No window (h = 0): crop images and masks are zeroed and none = rows cols.
 * crop_counts_or_null: HOST, (nframes - 1) x (2 + 2 radius) int64 with the fill's layout [none, own, -1, +1, ...]; with it the call waits
 * for the passes, without it they are only enqueued (the search's wait stays).
 * With stabilize_params_or_null->last_frame == 1 the inner call renders the last frame too (rsdsfm_stabilize.h), the crop search takes nframes
 * masks, rsdsfm_neighbour_poses is asked with nframes "pairs" and every per-frame loop runs p = 0 .. nframes - 1.  d_crop_images, d_crop_masks, d_crop_sources_or_null and crop_counts_or_null
 * then have nframes entries (rows), like the inner call's per-frame arrays; results, d_flows, seeds, the check masks, records and broken keep
 * nframes - 1 (nframes - 2 for the links).  The rule "byte for byte those public calls one after another" holds as it stands. */
int rsdsfm_stabilize_video_cropped_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                       double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                       const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows, double* const* d_depth_maps,
                                       double* const* d_R, double* const* d_t, rsdsfm_frame_result* results,
                                       const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks_or_null,
                                       const rsdsfm_link_params* link_params_or_null, rsdsfm_link_record* records, double* scales, double* A, double* c,
                                       uint8_t* broken_or_null, const rsdsfm_fuse_params* fuse_params_or_null, double* const* d_fused_maps_or_null,
                                       const rsdsfm_stabilize_params* stabilize_params_or_null, int mode, int q5_mode, int32_t iterations, double* A_s,
                                       double* c_s, double* M, double* m, uint8_t* const* d_stab_images, uint8_t* const* d_masks_out,
                                       int64_t* valid_or_null, const rsdsfm_stabilize_fill_params* fill_params_or_null, uint8_t* const* d_sources_or_null,
                                       int64_t* counts_or_null, const rsdsfm_stabilize_crop_params* crop_params_or_null, const int32_t* window_in_or_null,
                                       uint8_t* const* d_crop_images, uint8_t* const* d_crop_masks, uint8_t* const* d_crop_sources_or_null,
                                       int32_t window_out[4], int64_t* crop_counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_STABILIZE_CROP_H */
