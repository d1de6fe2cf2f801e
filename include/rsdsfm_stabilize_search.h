/*
 * rsdsfm_stabilize_search.h -- C ABI of the stabiliser's search for the VISIBLE pre-image on the MI355X: where the occlusion test
 * (rsdsfm_stabilize_visible.h) rejects a pixel of a neighbour's candidate, the neighbour usually did see the near surface; the fixed point is
 * started again from the source pixel that landed nearest the camera on that cell and the pixel is RECOVERED where that finds it.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  The
 * occlusion test detects a fold of a neighbour's map: stage C's p <- t - D(p), started at the target t, ends at the far pre-image, the
 * z-buffer holds something nearer, the pixel is rejected and left to the next candidate or to the inpainter -- so the near surface's
 * footprint at the frame border is invented, or taken from a frame further away, exactly where the stabiliser hides worst.  Here a tested
 * pixel has three outcomes, taken / recovered / rejected:
 *
 *   stage B++  stage B+ (D and zv keep their bytes) with the uint32 z-buffer replaced by a plane of uint64 KEYS on the virtual camera's grid,
 *              reset to all ones by a byte memset: every source pixel (y, x) that splats in stage B+ -- the same condition, the same cell --
 *              does kbuf[iy][ix] = min(., (uint64)bits(zv) << 32 | (y cols + x)): the nearest depth and, on equal depth, the smallest
 *              row-major source index; a 64-bit integer atomic minimum, exact and independent of scheduling.  kbuf >> 32 is stage B+'s zbuf
 *              wherever a pixel landed, 0xFFFFFFFF where that holds +inf.
 *   stage C++  p, `valid` and the first test exactly as rsdsfm_stabilize_visible_frame_dev's; zn is the high word of kn, the minimum key over
 *              the in-frame 3 x 3 block about the target's cell, an empty high word meaning "no evidence, visible".  A pixel that passes is
 *              TAKEN with that call's bytes.  A valid pixel with mask 0 that fails (a tap of zv is 0, or zs > zn k) takes the search:
 *              kn all ones: REJECTED.  Otherwise (sy, sx) = divmod(low word of kn, cols), q <- (sx, sy), `iterations` steps
 *              q <- t - bilinear(D, q) (the first fixed point's count and expressions), valid2 = its four comparisons on q, and the first
 *              test's decision at q against the same zn.  valid2 and passed: RECOVERED -- saturate_u8(bilinear(image, q)), mask 1, source
 *              source_id.  Otherwise REJECTED: image, mask and source keep what they had.
 * tests/stabilize_search_spec_numpy.py is the executable definition; the frame call reproduces it bit for bit.  DESIGN.md section 12
 * ("Visible pre-image") has the kernels, the launches, the bytes and what has been measured.
 *
 * In the clip calls the search is a knob of the context, rsdsfm_set_occlusion_search: with 1, rsdsfm_stabilize_video_filled_dev,
 * _cropped_dev, _blended_dev and, through the latter, _inpainted_dev make one rsdsfm_stabilize_search_frame_dev wherever they would make one
 * rsdsfm_stabilize_visible_frame_dev (rsdsfm_stabilize_fill_params.occlusion = 1, source ids >= 2), and "byte for byte those public calls
 * made one after another" holds with this call named.  The count arrays keep their layout: a recovered pixel counts under its offset.  With
 * occlusion = 0, or with the knob at 0, every byte of every clip call is what it is without this header.
 *
 * NOT here: the own frame (id 1) through the test, targets whose first fixed point leaves the frame, the dense rectifier's own folds,
 * per-clip recovered counts, a tolerance derived from the depth's error, the C++ mirror.
 */
#ifndef RSDSFM_STABILIZE_SEARCH_H
#define RSDSFM_STABILIZE_SEARCH_H

#include "rsdsfm_stabilize_visible.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One frame through a window, the occlusion test and the search: rsdsfm_stabilize_visible_frame_dev (its arguments, its rules, its errors)
 * with the third outcome above.
 * d_counts3_or_null: a DEVICE array [taken, rejected, recovered] of three int64, 8-byte aligned (else RSDSFM_ERR_INVALID); the call zeroes it
 * and the warp kernel itself adds to it (a sum per workgroup, three 64-bit integer atomics per workgroup: exact and independent of
 * scheduling) -- no launch is added.  taken is the visible call's taken, rejected + recovered its rejected.
 * kbuf and a zv of its own (12 B per pixel together; the visible call's planes are not touched) join the context's dense workspace on the
 * first call and on a size change and are released by rsdsfm_destroy; a context that never asks keeps its footprint.  kbuf is reset by a
 * byte memset on the context's stream in every call.  Dense, stabilise, fill, window, visible and search calls may alternate on one context.
 * Enqueued on the context's stream; returns without waiting. */
int rsdsfm_stabilize_search_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image_n, int32_t channels, const double* d_depth_n_colmajor, const double* d_R_n_rows9,
                                      const double* d_t_n_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int mode, int q5_mode,
                                      int32_t iterations, const double* M9, const double* m3, int32_t source_id, const int32_t window[4], uint8_t* d_image_inout,
                                      uint8_t* d_mask_inout, uint8_t* d_source_or_null, int32_t tol_q16, int64_t* d_counts3_or_null);

/* = rsdsfm_stabilize_window_launches(rows, cols): the map kernel splats the keys and the warp kernel tests, searches and counts by
 * themselves.  The memset of kbuf is not a kernel and is not counted.  Host only. */
int rsdsfm_stabilize_search_launches(int32_t rows, int32_t cols);

/* The clip calls' knob: 0 (the default) = a neighbour candidate that goes through the occlusion test goes through
 * rsdsfm_stabilize_visible_frame_dev, 1 = through rsdsfm_stabilize_search_frame_dev.  Anything else RSDSFM_ERR_INVALID.  It takes effect
 * only where rsdsfm_stabilize_fill_params.occlusion is 1.  Host only. */
int rsdsfm_set_occlusion_search(rsdsfm_ctx* ctx, int32_t on);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_STABILIZE_SEARCH_H */
