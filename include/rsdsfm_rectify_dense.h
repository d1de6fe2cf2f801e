/*
 * rsdsfm_rectify_dense.h -- C ABI of the DENSE global-shutter frame on the MI355X: a hole-free, sub-pixel rectified image from what the
 * solve already gives (the depth map of its inliers and the per-scanline pose table), for single frames and for whole clips.
 *
 * The forward splat (rsdsfm_rectify_frame_dev; rsframe.cc:803-839) moves every source pixel that has a depth to its nearest target
 * pixel: pixels without a depth (every non-inlier) land nowhere and the rest leave cracks.  Here
 *   A  the inverse depth rho = 1 / z of the valid pixels (z finite, z > 0) is filled over the whole frame by a push-pull pyramid (a cell of a
 *      coarser level is the mean of its non-zero children; a hole takes the bilinear value of the completed coarser level).  Valid
 *      pixels keep their z bit for bit; a filled pixel gets 1 / rho -- so a map whose valid depths all equal c fills to 1 / (1 / c), which is
 *      c itself for five doubles in six and one unit in the last place off otherwise, and filled depths lie within [min, max] of the valid
 *      ones up to that one rounding (the filled INVERSE depths lie within theirs exactly);
 *   B  every pixel runs the splat's chain (planeToSpace, cameraToWorldFrame(scanline), worldToCameraFrame(0), spaceToPlane) on the
 *      filled depth, which gives the displacement plane D(x, y) = (gx - x, gy - y), stored as two floats per pixel;
 *   C  every OUTPUT pixel g inverts that map by the fixed point p <- g - D(p) (D bilinear, replicate border; `iterations` steps) and takes
 *      the bilinear sample of the frame at p, rounded to nearest even.  mask = 1 where p lies within half a pixel of the frame, else the
 *      pixel and its mask are 0.  The marker colour (1, 1, 1) of the splat has no meaning here.  A map without a valid pixel gives all-zero
 *      outputs (decided on the device; no host wait).
 * tests/rectify_dense_spec_numpy.py is the executable definition; the kernels reproduce it bit for bit.  DESIGN.md section 12 has the stages,
 * the bytes per pixel, the launch count and the measured times.
 *
 * Alignment: frames, dense images and masks are read / written as packed 32-bit words: 4-byte aligned (RSDSFM_ERR_INVALID otherwise).
 */
#ifndef RSDSFM_RECTIFY_DENSE_H
#define RSDSFM_RECTIFY_DENSE_H

#include "rsdsfm_video.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One frame.  d_image rows x cols x channels bytes (channels 1 or 3), d_depth_map_colmajor rows x cols doubles as rsdsfm_depth_map_dev
 * writes them, d_R_rows9 / d_t_rows3 the pose table; mode RSDSFM_BACKPROJECT_RS / _GS and q5_mode as rsdsfm_back_project_dev;
 * iterations 1..16, 0 = the default (3).  Outputs: d_dense_image rows x cols x channels bytes; optional d_mask_or_null rows x cols
 * bytes (1 / 0), d_filled_depth_or_null rows x cols doubles, column-major like the input map, d_disp_or_null
 * rows x cols x 2 floats, row-major: stage B's D.  Enqueued on the context's stream; returns without waiting.  The pyramid (about 8 B x 1/3
 * per pixel) and the D plane (8 B per pixel) belong to the context: allocated on first use and when the size changes, released by
 * rsdsfm_destroy.  RSDSFM_ERR_INVALID: rows or cols outside [2, 16384], an unknown mode / q5_mode, iterations outside 0..16, channels other
 * than 1 or 3, a NULL required pointer, d_dense_image == d_image, a misaligned image or mask. */
int rsdsfm_rectify_dense_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, int32_t channels, const double* d_depth_map_colmajor,
                                   const double* d_R_rows9, const double* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows,
                                   int32_t cols, int mode, int q5_mode, int32_t iterations, uint8_t* d_dense_image, uint8_t* d_mask_or_null,
                                   double* d_filled_depth_or_null, float* d_disp_or_null);

/* A whole clip: rsdsfm_solve_video_dev (its arguments up to `results`, its results, its rules, its errors) and, behind the solve of every
 * pair p on that pair's lane and with that lane's workspace, the dense rectification of frame p with pair p's depth map and pose table.
 * Per-pair outputs, nframes - 1 device pointers each: d_dense_images[p] rows x cols x channels bytes, d_masks_or_null[p] rows x cols bytes,
 * d_filled_depths_or_null[p] rows x cols doubles (either array may be NULL) -- bit for bit what rsdsfm_rectify_dense_frame_dev writes from
 * d_frames[p], d_depth_maps[p] and pair p's pose table, at every batch size and lane count.  Pose tables as rsdsfm_rectify_video_dev (a
 * lane-owned scratch table where d_R_or_null / d_t_or_null is NULL).  Synchronous in its outputs: it waits for every lane.  Errors as
 * rsdsfm_rectify_video_dev's, "pair i: ..." numbered within the clip. */
int rsdsfm_rectify_dense_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                   double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                   const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows_or_null,
                                   double* const* d_depth_maps, double* const* d_R_or_null, double* const* d_t_or_null, rsdsfm_frame_result* results,
                                   int mode, int q5_mode, int32_t iterations, uint8_t* const* d_dense_images, uint8_t* const* d_masks_or_null,
                                   double* const* d_filled_depths_or_null);

/* Kernel launches rsdsfm_rectify_dense_frame_dev enqueues for a rows x cols frame (4 while every pyramid level from level 1 up fits one
 * workgroup's LDS, 9 at 1280 x 720; the copy of d_disp_or_null is not counted), or RSDSFM_ERR_INVALID for a size outside [2, 16384].  Host only. */
int rsdsfm_rectify_dense_launches(int32_t rows, int32_t cols);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_RECTIFY_DENSE_H */
