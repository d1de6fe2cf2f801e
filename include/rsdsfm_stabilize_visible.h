/*
 * rsdsfm_stabilize_visible.h -- C ABI of the stabiliser's occlusion test on the MI355X: a neighbour frame rendered into a virtual camera
 * offers a pixel only when the source pixel stage C found is the one nearest the camera among those that land there.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  The
 * border fill (rsdsfm_stabilize_fill.h), the crop (rsdsfm_stabilize_crop.h) and the seam blend (rsdsfm_stabilize_blend.h) all render
 * neighbour n into the virtual camera of frame q the same way: stage C inverts the displacement plane D by p <- t - D(p) from p = t.  Where
 * the neighbour's map FOLDS -- a near surface has moved in front of a far one under the baseline between n and q~ -- a target has two
 * pre-images and the iteration finds the one nearer in the image plane, not the one nearer the camera: the far surface is painted inside
 * the near one's footprint, a parallax ghost that sits at the frame border and differs from frame to frame.  Here such a pixel is REJECTED;
 * the next candidate, or the inpainter, takes it.
 *
 *   stage B+  stage B as it is (D keeps its bytes) and two planes: zv, float32 on the source grid, (float)pv[2] where pv[2] > 0 and finite
 *             and the float is finite, else 0 (pv: the point in the virtual camera, the value the existing chain computes); and the
 *             z-buffer zbuf, uint32 on the VIRTUAL CAMERA's own pixel grid (whatever window is used later), reset to 0x7f800000 (+inf):
 *             every source pixel with zv > 0, -0.5 <= gx < cols - 0.5 and -0.5 <= gy < rows - 0.5 does zbuf[iy][ix] = min(., bits(zv)),
 *             ix = min((int)(gx + 0.5), cols - 1), iy likewise, with the projection's doubles gx, gy.  Positive floats order as their bit
 *             patterns: an integer atomic minimum, exact and independent of scheduling.
 *   stage C+  p and `valid` exactly as rsdsfm_stabilize_window_frame_dev's for target t.  A valid pixel whose mask byte is 0 takes the
 *             test: zs = the bilinear sample of zv at the image sample's taps, in double -- any tap 0: rejected; zn = the minimum of zbuf
 *             over the in-frame part of the 3 x 3 block about (ic, jc), jc = (int)min(max(tx + 0.5, 0), cols - 1), ic likewise.
 *             zn == +inf: nothing was splatted there, no evidence, visible.  Otherwise rejected iff zs > (double)zn k,
 *             k = 1.0 + tol_q16 / 65536.0, computed once on the host.
 * The 3 x 3 block covers the splat's cracks and the float rounding of D; it erodes a depth edge by one pixel.  The default tolerance,
 * tol_q16 = 3277 (about 0.05), is a choice, not a measurement.
 * tests/stabilize_visible_spec_numpy.py is the executable definition; the frame call reproduces it bit for bit.  DESIGN.md section 12
 * ("Occlusion test") has the kernels, the launches, the bytes and what has been measured.
 *
 * In the clip calls the test is asked for with rsdsfm_stabilize_fill_params.occlusion = 1 (rsdsfm_stabilize_fill.h): the neighbour
 * candidates (source ids >= 2) of rsdsfm_stabilize_video_filled_dev, _cropped_dev, _blended_dev and, through the latter, _inpainted_dev
 * then go through rsdsfm_stabilize_visible_frame_dev -- the filled call with the window (0, 0, rows, cols) -- and "byte for byte those
 * public calls made one after another" holds with this call named in the others' place.  The own frame (id 1) keeps its call.  The count
 * arrays keep their layout: a rejected pixel shows up as fewer pixels for that offset and more for later offsets or `none`.
 *
 * NOT here: searching for the VISIBLE pre-image instead of rejecting (built since: rsdsfm_stabilize_search.h), the own frame, the dense rectifier's own folds, per-clip rejected
 * counts, the C++ mirror.
 */
#ifndef RSDSFM_STABILIZE_VISIBLE_H
#define RSDSFM_STABILIZE_VISIBLE_H

#include "rsdsfm_stabilize_crop.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSDSFM_OCCLUSION_TOL_Q16_DEFAULT 3277 /* about 0.05 of the depth: a choice, not a measurement */

/* One frame through a window and the occlusion test: rsdsfm_stabilize_window_frame_dev (its arguments, its rules, its errors; source_id
 * 1 .. 255) with the decision above between stage C's validity and the write: a rejected pixel is not taken -- image, mask and source keep
 * what they had.  Pixels whose mask byte is already set are neither tested nor counted; a candidate without one valid depth offers nothing
 * and counts nothing.
 * tol_q16: 0 = the default, 1 .. 65536; anything else RSDSFM_ERR_INVALID.
 * d_counts2_or_null: a DEVICE array [taken, rejected] of two int64, 8-byte aligned (else RSDSFM_ERR_INVALID); the call zeroes it and the
 * warp kernel itself adds to it (a sum per workgroup, two 64-bit integer atomics per workgroup: exact and independent of scheduling) -- no
 * launch is added.  It stands where rsdsfm_stabilize_window_frame_dev has d_filled_or_null.
 * zv and zbuf (8 B per pixel together) join the context's dense workspace on the first call and on a size change and are released by
 * rsdsfm_destroy; a context that never asks keeps its footprint.  zbuf is reset by a 4-byte memset on the context's stream in every call.
 * Dense, stabilise, fill, window and visible calls may alternate on one context.  Enqueued on the context's stream; returns without
 * waiting. */
int rsdsfm_stabilize_visible_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image_n, int32_t channels, const double* d_depth_n_colmajor, const double* d_R_n_rows9,
                                       const double* d_t_n_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int mode, int q5_mode,
                                       int32_t iterations, const double* M9, const double* m3, int32_t source_id, const int32_t window[4], uint8_t* d_image_inout,
                                       uint8_t* d_mask_inout, uint8_t* d_source_or_null, int32_t tol_q16, int64_t* d_counts2_or_null);

/* = rsdsfm_stabilize_window_launches(rows, cols): the map kernel splats and the warp kernel tests and counts by themselves.  The memset of
 * zbuf is not a kernel and is not counted.  Host only. */
int rsdsfm_stabilize_visible_launches(int32_t rows, int32_t cols);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_STABILIZE_VISIBLE_H */
