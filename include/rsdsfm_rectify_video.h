/*
 * rsdsfm_rectify_video.h -- C ABI of the rectified products of whole clips on the MI355X: consecutive 8-bit frames -> per pair the
 * solve (include/rsdsfm_video.h) AND what evaluateSingleRun makes of it (main.cc:480-523): the 8-bit depth image, the global-shutter
 * image, the crack-interpolated image and the world points -- for BGR frames and for one-channel (gray) frames.
 *
 * A gray value g stands for the BGR pixel (g, g, g); the gray outputs are channel 0 of what the BGR rectifier produces for that
 * replicated image.  The rectifier's three rules are symmetric in the channels -- the marker colour (1, 1, 1) that backProject skips
 * (rsframe.cc:816) is g == 1; "black" (cv::norm(Vec3b) <= 15, camera.cc:694) is 3 g^2 <= 225, i.e. g <= 8; a black pixel takes
 * saturate_u8(sum / count) over its non-black 4-neighbours -- so this is well defined.  The depth image and the world points do not
 * depend on the channel count.  DESIGN.md section 12 ("Sequences") has the measured times.
 *
 * Alignment: the kernels store four pixels as packed 32-bit words, so every image buffer (frames, global-shutter and interpolated
 * images, BGR or gray) and the world points must be 4-byte aligned, as rsdsfm_rectify_frame_dev's; depth images may have any alignment.
 * Less is refused with RSDSFM_ERR_INVALID before anything is enqueued (include/rsdsfm.h, "Alignment of device pointers").
 */
#ifndef RSDSFM_RECTIFY_VIDEO_H
#define RSDSFM_RECTIFY_VIDEO_H

#include "rsdsfm_video.h"

#ifdef __cplusplus
extern "C" {
#endif

/* main.cc:480-523 (rsframe.cc:803-878, camera.cc:694-774) on a ONE-channel image: rsdsfm_rectify_frame_dev's arguments, with d_image,
 * d_gs_image and d_fixed_image rows x cols bytes.  d_gs_image / d_fixed_image are channel 0 of what rsdsfm_rectify_frame_dev writes
 * for the image (g, g, g); d_depth_est and d_coords3d_or_null are that call's, bit for bit.  Same launches (two; three when offset > 2
 * or cols is not a multiple of 4), 1 B + 8 B read and 1 B + 1 B + 12 B written per pixel instead of 3 B + 8 B and 3 B + 3 B + 12 B.
 * Enqueued on the context's stream; returns without waiting.  Errors as rsdsfm_rectify_frame_dev (d_gs_image == d_fixed_image too). */
int rsdsfm_rectify_gray_frame_dev(rsdsfm_ctx* ctx, const double* d_inl, int64_t m, const uint8_t* d_image, const double* d_depth_map,
                                  const double* d_R_rows9, const double* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                                  int mode, int q5_mode, int32_t offset, uint8_t* d_depth_est, uint8_t* d_gs_image, float* d_coords3d_or_null,
                                  uint8_t* d_fixed_image);

/* camera.cc:253-277 + main.cc:380-523 for a whole clip: rsdsfm_solve_video_dev (its arguments up to `results`, its results, its rules
 * for the device pointers inside them, its errors) and, behind the solve of every pair p on that pair's lane, the rectification of
 * frame p with pair p's solve.  mode / q5_mode / offset as rsdsfm_rectify_frame_dev; per-pair outputs, nframes - 1 device pointers
 * each: d_depth_est[p] rows x cols bytes, d_gs_images[p] and d_fixed_images[p] rows x cols x channels bytes, d_coords3d_or_null[p]
 * rows x cols x 3 floats (the array may be NULL).  They are bit for bit what rsdsfm_rectify_frame_dev (channels == 1:
 * rsdsfm_rectify_gray_frame_dev) writes from results[p].d_inliers / num_inliers, d_frames[p], d_depth_maps[p] and pair p's pose
 * table, at every batch size and lane count.  Where d_R_or_null / d_t_or_null is NULL the table lives in a scratch buffer of the
 * pair's lane (rows x 12 doubles per lane, owned by the context); a table array that is passed is written for every pair, even when
 * the other one is NULL.  Synchronous in its outputs: ALL of them are complete when the call returns (it waits for every lane).
 * RSDSFM_ERR_INVALID for everything rsdsfm_solve_video_dev and rsdsfm_rectify_frame_dev refuse: nframes < 2, a NULL inside a required
 * array, channels other than 1 or 3, an unknown mode / q5_mode, offset < 0, d_gs_images[p] == d_fixed_images[p].  Errors of a pair
 * read "pair i: ...", numbered within the clip. */
int rsdsfm_rectify_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels, double fx,
                             double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                             const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows_or_null, double* const* d_depth_maps,
                             double* const* d_R_or_null, double* const* d_t_or_null, rsdsfm_frame_result* results, int mode, int q5_mode, int32_t offset,
                             uint8_t* const* d_depth_est, uint8_t* const* d_gs_images, uint8_t* const* d_fixed_images, float* const* d_coords3d_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_RECTIFY_VIDEO_H */
