/*
 * rsdsfm_superres.h -- C ABI of the multi-frame super-resolution on the MI355X: a frame of a solved clip on a grid S times finer than its
 * source (S 1 .. 4), merged from the own frame and its neighbours in time, every one rendered ALONE into the frame's own (virtual) camera on
 * the fine grid through its depth map and rolling-shutter pose table.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  Every
 * other stage of the clip pipeline keeps the input's sample count; the crop-and-zoom magnifies one frame by one bilinear interpolation.
 * Hand-held shake puts the neighbours' samples at different sub-pixel phases of the same surface, and the clip is already registered in 3-D.
 *   render      one source onto orows x ocols = S rows x S cols (both at most 16384) through the window (r0, c0, h, w) of the crop stage:
 *               target of output pixel (X, Y): tx = (c0 + (X + 0.5) (w / ocols)) - 0.5, ty = (r0 + (Y + 0.5) (h / orows)) - 0.5; stages A and
 *               B (depth fill, displacement plane D) are the existing launches on the SOURCE grid; stage C is the existing fixed point
 *               p = t, p <- t - bilinear(D, p) and validity test.  With the taps (i0, i1, a) of p per axis, three planes:
 *                 bil   the existing bilinear sample (saturate_u8 of the two lerps), orows x ocols x channels
 *                 near  the source byte at (a_y < 0.5 ? i0 : i1, a_x < 0.5 ? i0 : i1), same size
 *                 prox  1 + (int) floor(15 ((1 - 2 d_x) (1 - 2 d_y))), d = min(a, 1 - a) per axis: 16 on a source sample, 1 half way between
 *                       two on either axis; orows x ocols
 *               all 0 where p is not valid, and all-zero planes for a source without a valid depth.  prox is the planes' mask in the
 *               project's "set iff not 0" sense: rsdsfm_seam_overlap_sums_dev takes bil and prox as a layer image and its mask.  At S = 1 bil
 *               and prox != 0 are byte for byte rsdsfm_stabilize_window_frame_dev's image and mask on zeroed planes.
 *   accumulate  reference = the own frame's planes (R = bil, RN = near, qR = prox), layer = a neighbour's (B, Nn, qL).  Gains G_c from the
 *               8-word record and k(x) = min(255, (G_c x + 32768) >> 16) exactly as in rsdsfm_denoise.h.  v = qR != 0 and qL != 0;
 *               e = sum_c |R_c - k(B_c)| where v; D, N the 3 x 3 sums of e and of channels v inside the frame;
 *               w = 16 - min(16, (16 D) / (h N)) where v, else 0 (the denoise's patch weight, on the bilinear samples);
 *               u = (w qL + 8) >> 4, 0 .. 16.
 *   cell        per fine pixel, BGR: four uint16 [s_b, s_g, s_r, n] (8 B); gray: two uint16 [s, n] (4 B): rsdsfm_shutter.h's layout.
 *               first      the cell is [qR RN_c, qR] (all 0 where qR == 0; what it held never shows); then the layer is added
 *               every step s_c += u k(Nn_c), n += u
 *               not last   the cells are written
 *               last       the cells are NOT written; where n > qR out_c = (2 s_c + n) / (2 n) (round half up); where n == qR > 0
 *                          out_c = R_c -- a pixel no neighbour contributed to is the bilinear upscale, not a blocky nearest one --; else 0.
 *                          mask = n > 0, the weight plane is n, the counters [unset, own only: n == qR > 0, merged: n > qR]
 *               With at most RSDSFM_SUPERRES_LAYERS_MAX = 14 layers n <= 240 and s_c <= 61 200: nothing overflows.  THE CALLER OF
 *               rsdsfm_superres_accumulate_dev KEEPS TO 14 LAYERS per `first` and to planes with prox <= 16; the call cannot check either.
 *   frame       source 0 (the own frame) and every neighbour rendered alone; per neighbour the record by rsdsfm_seam_overlap_sums_dev from
 *               (R, the own frame's validity plane, B, qL), then one accumulate.
 * The sums are integers: the result does not depend on the order of the layers, and a layer that disagrees with the own frame everywhere
 * (w = 0) leaves R's bytes exactly.  Positions are float64 with one rounding per operation, everything after the render is integers;
 * tests/superres_spec_numpy.py is the executable definition and every call here reproduces it bit for bit.  DESIGN.md section 12
 * ("Super-resolution") has the kernels, the bytes, the launches and the LDS layout.
 *
 * CHOICES, NOT MEASUREMENTS: the proximity weight, the nearest-sample values, the 3 x 3 patch on the fine grid, and the defaults (scale 2,
 * radius 2, strength 12).  Measured on the CPU only (a pure-translation clip of five frames; tests/test_superres_cpu.py): the mean absolute
 * error against the fine-grid truth is 0.66 - 0.67 of the bilinear upscale's at S = 2 and 0.79 - 0.84 at S = 3.  Tried and rejected there:
 * accumulating each neighbour's BILINEAR sample gains nothing (0.97 - 1.02); the patch test on nearest samples rejects good neighbours.
 *
 * NOT here: neighbours through the occlusion test or the search (their z-buffer lives on the coarse grid; a neighbour that disagrees falls
 * back to the own pixel through w), deconvolution or sharpening of the sensor blur, non-integer scales, a fused render-and-accumulate, fill,
 * blend or inpaint of the result, the C++ mirror.
 */
#ifndef RSDSFM_SUPERRES_H
#define RSDSFM_SUPERRES_H

#include "rsdsfm_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSDSFM_SUPERRES_SCALE_MAX 4
#define RSDSFM_SUPERRES_RADIUS_MAX 7
#define RSDSFM_SUPERRES_LAYERS_MAX 14
#define RSDSFM_SUPERRES_PROX_MAX 16
/* the defaults: choices, not measurements */
#define RSDSFM_SUPERRES_SCALE_DEFAULT 2
#define RSDSFM_SUPERRES_RADIUS_DEFAULT 2
#define RSDSFM_SUPERRES_STRENGTH_DEFAULT 12

typedef struct rsdsfm_superres_params {
    int32_t scale;        /* S, 1 .. 4; 0: the default, 2 */
    int32_t radius;       /* neighbours on each side for the clip call, 1 .. 7; 0: the default, 2 */
    int32_t strength;     /* h, 1 .. 255; 0: the default, 12 */
    int32_t gain_mode;    /* 0: every neighbour gain-matched to the own frame on their overlap, the default; 1: off */
    int64_t min_overlap;  /* overlap (fine) pixels below which a neighbour gets no gain, >= 0; 0: the default, 1024 (the blend's) */
    int32_t struct_bytes; /* 0 or sizeof(rsdsfm_superres_params), as rsdsfm_superres_params_init sets it; anything else is refused */
    int32_t reserved[5];  /* 0 */
} rsdsfm_superres_params;

/* scale = 2, radius = 2, strength = 12, gain_mode = 0, min_overlap = 1024, struct_bytes = sizeof.  A NULL params pointer means these values. */
int rsdsfm_superres_params_init(rsdsfm_superres_params* params);

/* One source rendered alone onto the fine grid, as defined above.  d_image_n (rows x cols x channels bytes, channels 1 or 3, 4-byte aligned),
 * d_depth_n_colmajor, d_R_n_rows9, d_t_n_rows3, the camera, rows, cols (the SOURCE size, each in [2, 16384]), mode, q5_mode, iterations, M9, m3
 * and window (r0, c0, h, w on the source grid; NULL: the full frame) are rsdsfm_stabilize_window_frame_dev's.  scale 1 .. 4 with scale * rows
 * and scale * cols at most 16384.  Outputs, DEVICE, 4-byte aligned, distinct from each other and from the image, every byte written (no
 * preset): d_bil_out and d_near_out (scale rows x scale cols x channels), d_prox_out (scale rows x scale cols), and d_valid_or_null (scale rows
 * x scale cols: 1 where prox != 0, else 0 -- the source plane rsdsfm_seam_overlap_sums_dev wants beside the own frame's bil, whose selector is
 * `== 1`; NULL: not written).
 * Enqueues stage A and stage B on the source grid (the existing launches, into the context's dense workspace) and one launch of
 * superres_warp_kernel<CH> on the context's stream; returns without waiting.  A refused call enqueues nothing.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased pointer, channels, a size or scale outside its range, a non-finite pose, a window outside
 * the frame, and what rsdsfm_stabilize_window_frame_dev refuses of mode, q5_mode and iterations. */
int rsdsfm_superres_render_dev(rsdsfm_ctx* ctx, const uint8_t* d_image_n, int32_t channels, const double* d_depth_n_colmajor, const double* d_R_n_rows9,
                               const double* d_t_n_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int mode, int q5_mode,
                               int32_t iterations, const double* M9, const double* m3, int32_t scale, const int32_t* window_or_null, uint8_t* d_bil_out,
                               uint8_t* d_near_out, uint8_t* d_prox_out, uint8_t* d_valid_or_null);

/* = rsdsfm_stabilize_window_launches(rows, cols): stages A and B and one warp.  RSDSFM_ERR_INVALID for a size or scale outside its range.
 * Host only. */
int rsdsfm_superres_render_launches(int32_t rows, int32_t cols, int32_t scale);

/* One step, as defined above, on FINE planes of rows x cols (each in [2, 16384]); the call knows nothing of the scale.  d_ref_bil, d_ref_near,
 * d_layer_bil_or_null, d_layer_near_or_null: rows x cols x channels bytes, channels 1 or 3; d_ref_prox, d_layer_prox_or_null: rows x cols
 * bytes, 0 .. 16; DEVICE, only read.  The three layer pointers are all given or all NULL; NULL (no layer) needs first == 1 and last == 1.
 * d_sums8_or_null: the layer's record on the DEVICE, 8-byte aligned, only read -- every workgroup computes the gains from it itself, so no
 * host wait stands between rsdsfm_seam_overlap_sums_dev and this call; NULL: no gain.  min_overlap >= 0 (0: 1024), gain_mode 0 / 1, strength
 * 1 .. 255 (0: 12).  d_cells_or_null: rows x cols cells, DEVICE, 8-byte aligned; NULL only with first && last.  first, last: 0 or 1.
 * d_image_out, d_mask_out, d_weight_or_null (rows x cols bytes), d_counts3_or_null are read only when last, and then every byte of the output
 * planes is written, so they need no preset.  d_counts3_or_null: a DEVICE array [unset, own only, merged] of three int64, 8-byte aligned; the
 * call zeroes it (a memset on the context's stream) and the kernel adds to it -- a sum per workgroup with shuffles and LDS, then three 64-bit
 * integer atomics per workgroup: exact and independent of scheduling.
 * Every plane is 4-byte aligned; the outputs are distinct from the inputs, from the cells and from each other, the cells from the inputs.
 * One kernel launch (superres_accumulate_kernel<CH, FIRST, LAST>), enqueued on the context's stream; returns without waiting.  A refused call
 * enqueues nothing.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased pointer, only some of the three layer pointers, no layer without first && last, channels,
 * a size outside [2, 16384], first or last other than 0 / 1, min_overlap < 0, gain_mode, strength outside its range. */
int rsdsfm_superres_accumulate_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_bil, const uint8_t* d_ref_near, const uint8_t* d_ref_prox,
                                   const uint8_t* d_layer_bil_or_null, const uint8_t* d_layer_near_or_null, const uint8_t* d_layer_prox_or_null, int32_t channels,
                                   int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null, int64_t min_overlap, int32_t gain_mode, int32_t strength,
                                   uint16_t* d_cells_or_null, int32_t first, int32_t last, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null,
                                   int64_t* d_counts3_or_null);

/* Kernel launches of rsdsfm_superres_accumulate_dev: 1.  The memset of the counters is not counted.  Host only. */
int rsdsfm_superres_accumulate_launches(void);

/* One super-resolved frame.  d_images, d_depths_colmajor, d_R_rows9, d_t_rows3: HOST arrays of nsrc DEVICE pointers, as rsdsfm_denoise_frame_dev
 * takes them; the camera, rows, cols (the SOURCE size), mode, q5_mode and iterations are that call's.  nsrc 1 .. 15: source 0 is the own frame,
 * the others its neighbours.  M (nsrc x 9, row-major) and m (nsrc x 3): HOST, every source's pose in the target camera (rsdsfm_retime_poses'
 * for the own frame, rsdsfm_neighbour_poses' for the others).  window_or_null: (r0, c0, h, w) on the source grid, NULL = the full frame.  The
 * outputs are FINE planes: d_image_out (S rows x S cols x channels), d_mask_out, d_weight_or_null (S rows x S cols), S = params->scale.
 * In order, on the context's stream:
 *   1. the own frame by rsdsfm_superres_render_dev into the context's own planes, with the validity plane;
 *   2. per neighbour: rsdsfm_superres_render_dev into the context's layer planes (no validity plane); rsdsfm_seam_overlap_sums_dev(own bil, own
 *      validity plane, layer bil, layer prox) into the record; rsdsfm_superres_accumulate_dev (first on the first neighbour, last on the last);
 *   3. with nsrc == 1 a single rsdsfm_superres_accumulate_dev with no layer: the image is the own frame's bil, the mask prox != 0.
 * Every output is byte for byte those public calls made one after another.  The own planes (2 channels + 2 B per fine pixel: bil, near, prox
 * and the validity plane), the layer planes (2 channels + 1 B), the record and the cells (8 B per fine pixel) join the context's workspace with
 * the first call and after a change of size or scale and are released by rsdsfm_destroy: a context that never asks keeps its footprint.
 * params->radius is not read here.  Returns without waiting.
 * RSDSFM_ERR_INVALID: nsrc outside [1, 15], a NULL array or entry, a misaligned source image, a source image that is an output, a NULL or
 * non-finite M / m, scale, strength, gain_mode, min_overlap or radius outside its range, bad struct_bytes, non-zero reserved words, and the
 * lists of rsdsfm_superres_render_dev and rsdsfm_superres_accumulate_dev. */
int rsdsfm_superres_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                              const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                              int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_superres_params* params_or_null,
                              const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, int64_t* d_counts3_or_null);

/* = nsrc rsdsfm_superres_render_launches(rows, cols, scale) + 2 (nsrc - 1) (the sums and the accumulate per neighbour), or + 1 when nsrc == 1.
 * RSDSFM_ERR_INVALID for a size or scale outside its range or nsrc outside [1, 15].  Host only. */
int rsdsfm_superres_launches(int32_t rows, int32_t cols, int32_t scale, int32_t nsrc);

/* A clip, super-resolved AFTER it was solved: the call reads what rsdsfm_stabilize_video_dev or one of its variants left behind, exactly as
 * rsdsfm_denoise_video_dev does (same arrays, same walk): for q = 0 .. nsources - 1 in order the own pose by rsdsfm_retime_poses(t = q), the
 * neighbours and their poses by rsdsfm_neighbour_poses(q, params->radius) on the same path, then rsdsfm_superres_frame_dev into
 * d_out_images[q], d_out_masks[q] and d_out_weights_or_null[q] (FINE planes; the array may be NULL).  All poses are computed before anything
 * is enqueued.  Every plane is byte for byte what the frame calls give when made one after another.  counts_or_null: HOST, nsources x 3 int64
 * [unset, own only, merged]; with it the call ends with one copy and one wait, without it the call only enqueues.
 * RSDSFM_ERR_INVALID: a NULL array or entry, nsources < 1, an output plane that is a frame of the clip, what rsdsfm_retime_poses or
 * rsdsfm_neighbour_poses refuses, and the frame call's list. */
int rsdsfm_superres_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                              double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                              const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                              const rsdsfm_superres_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks,
                              uint8_t* const* d_out_weights_or_null, int64_t* counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_SUPERRES_H */
