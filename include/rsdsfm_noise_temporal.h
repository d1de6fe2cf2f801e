/*
 * rsdsfm_noise_temporal.h -- C ABI of the temporal noise curve on the MI355X: one frame's noise measured from the differences to its
 * REGISTERED NEIGHBOURS, in the noise curve's format (rsdsfm_noise_curve.h, which this header includes), and the temporal denoise and the
 * spatial top-up at the strength per pixel that curve asks for.
 *
 * rsdsfm_noise_curve.h applies Immerkaer's 3 x 3 mask to ONE frame and so assumes that most of the frame is smooth: on a textured frame it
 * measures the texture, its strength opens the temporal gate completely and a mover ghosts.  The difference of two registered renders of a
 * static scene holds no texture.  The reference has no counterpart.  tests/noise_temporal_spec_numpy.py is the executable definition; every
 * call here reproduces it bit for bit.  Integers only.
 *   pair        the reference R with its mask mR and one neighbour's layer L with its mask mL, rendered alone into R's camera; the gains G
 *               and k = gained(L, G) exactly as in rsdsfm_denoise.h.
 *   valid       v(p) = mR(p) != 0 and mL(p) != 0;  e(p) = sum_c |R_c(p) - k_c(p)| where v, else 0;
 *               clipped(p) = v and any byte of R(p) or of L(p) BEFORE the gain is 0 or 255.
 *   sample      D, C, X = the 3 x 3 sums of e, v, clipped about p (0 outside the frame).  p is a sample iff C = 9 and X = 0: a full window, so
 *               an interior pixel, with nothing saturated.  D is the sum the temporal weight thresholds.
 *   bin         N = 9 channels; bin = (918 D + 128 N) / (256 N) <= 914: the patch mean times 918 / 256, rounded half up.
 *               918 / 256 = 3.586 is derived: Immerkaer's m is 0.6745 * 6 sigma = 4.047 sigma, E|R - k| = 2 sigma / sqrt(pi) = 1.128 sigma
 *               for equal Gaussian noise in both frames, and 4.047 / 1.128 = 3.586.  So m, sigma_q8 and h = (scale m + 8) >> 4 keep the
 *               meaning they have in rsdsfm_noise.h.
 *   band        level(R(p)) >> 5 with the consumers' level: the byte (gray) or (b + g + r + 1) / 3 (BGR).
 *   histogram   hist[band][bin] += 1: rsdsfm_noise_curve.h's 8 x 1024 uint32.  A frame's histogram is the sum over all its neighbours:
 *               integers, so exact and independent of the neighbours' order and of scheduling.
 *   curve       rsdsfm_noise_curve.h's 36 words from that histogram, by its own resolve kernel.  Every consumer of a curve takes it unchanged:
 *               rsdsfm_denoise_accumulate_curve_dev, rsdsfm_denoise_spatial_curve_dev, rsdsfm_sharpen_curve_dev, rsdsfm_noise_curve_strengths.
 * DESIGN.md section 12 ("Temporal noise curve") has the kernel, the LDS layout, the resources and the measurements.
 *
 * NOT here: the temporal curve fed to rsdsfm_sharpen_frame_dev (the noise after denoising is not the noise measured before it), a curve
 * consumer for the super-resolution and for the sharpness transfer, histograms pooled across the frames of a clip, a fallback to the spatial
 * curve when the overlap is too small, Solver methods and package-level names, the C++ mirror, the fuzz campaign entry.
 */
#ifndef RSDSFM_NOISE_TEMPORAL_H
#define RSDSFM_NOISE_TEMPORAL_H

#include "rsdsfm_noise_curve.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One neighbour's pair histogram as defined above.  The reference, the layer, channels, rows, cols, d_sums8_or_null (the overlap record, NULL:
 * no gain), min_overlap (0: the default, 1024) and gain_mode: as rsdsfm_denoise_accumulate_dev takes them; the layer is required.
 * d_hist8192: 8 x 1024 uint32 on the DEVICE, 4-byte aligned, distinct from every input.  first = 1: a memset zeroes the histogram in front of
 * the launch, so it needs no preset; first = 0: the launch adds to what it holds.  rows, cols in [2, 16384].
 * Enqueues the memset (with first) and ONE launch on the context's stream -- noise_pair_hist_kernel<CH>, one 32-bit integer atomicAdd per
 * non-zero bin and workgroup -- and returns without waiting.
 * RSDSFM_ERR_INVALID with a "noise pair: ..." message and nothing enqueued: a NULL, misaligned or aliased pointer, channels, a size,
 * min_overlap < 0, gain_mode or first outside {0, 1}. */
int rsdsfm_noise_pair_hist_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image, const uint8_t* d_layer_mask,
                               int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null, int64_t min_overlap, int32_t gain_mode, int32_t first,
                               uint32_t* d_hist8192);

/* Kernel launches of rsdsfm_noise_pair_hist_dev: 1.  The memset is not counted.  Host only. */
int rsdsfm_noise_pair_hist_launches(void);

/* The curve of a histogram: rsdsfm_noise_curve_dev's second launch alone (noise_curve_resolve_kernel, nine independent workgroups).
 * d_hist8192: 8 x 1024 uint32 on the DEVICE, 4-byte aligned, only read; quantile_q8 in [1, 256], 0: the default, 128; d_curve36_out: 36 uint64
 * on the DEVICE, 8-byte aligned, every word written, not the histogram.  On the histogram rsdsfm_noise_curve_dev wrote it gives that call's
 * curve byte for byte.  One launch on the context's stream; returns without waiting.
 * RSDSFM_ERR_INVALID with a "noise resolve: ..." message and nothing enqueued: a NULL, misaligned or aliased pointer, the quantile. */
int rsdsfm_noise_curve_resolve_dev(rsdsfm_ctx* ctx, const uint32_t* d_hist8192, int32_t quantile_q8, uint64_t* d_curve36_out);

/* Kernel launches of rsdsfm_noise_curve_resolve_dev: 1.  Host only. */
int rsdsfm_noise_curve_resolve_launches(void);

/* rsdsfm_denoise_curve_frame_dev with the curve measured from the registered neighbours: exactly its arguments.  In order, on the context's
 * stream: the own render; per neighbour j its render alone onto layer j of a stack in the workspace, the overlap record j, and
 * rsdsfm_noise_pair_hist_dev with first on j = 0; ONE rsdsfm_noise_curve_resolve_dev with curve->quantile_q8; per neighbour
 * rsdsfm_denoise_accumulate_curve_dev on its layer, its record and that curve (params->strength is the fallback); with spatial_or_null
 * rsdsfm_denoise_spatial_curve_dev on the same curve.  With one source the histogram is empty, row 8 has n = 0 and every strength is the
 * fallback.  The stack (channels + 1 bytes per pixel and neighbour) and the records join the dense workspace with the first call, grow when a
 * call needs more, and are released by rsdsfm_destroy.  Every output is byte for byte the public calls made one after another; whatever any of
 * them would refuse is refused before the first enqueue.  Returns without waiting.
 * RSDSFM_ERR_INVALID ("denoise temporal frame: ..."): rsdsfm_denoise_curve_frame_dev's list. */
int rsdsfm_denoise_temporal_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                                      const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                                      int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_denoise_params* params_or_null,
                                      const rsdsfm_noise_curve_params* curve_or_null, const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null,
                                      uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, uint8_t* d_support_or_null, int64_t* d_counts6_or_null,
                                      uint64_t* d_curve36_or_null);

/* = rsdsfm_denoise_launches(rows, cols, nsrc) + (nsrc - 1) pair histograms + 1 resolve, + 1 more with the top-up (with_spatial != 0), and
 * its refusals.  Host only. */
int rsdsfm_denoise_temporal_frame_launches(int32_t rows, int32_t cols, int32_t nsrc, int32_t with_spatial);

/* rsdsfm_denoise_curve_video_dev's arguments and walk with rsdsfm_denoise_temporal_frame_dev per frame.  counts_or_null: HOST, nsources x 6
 * int64; noise_curves_or_null: HOST, nsources x 36 uint64, every frame's curve.  With either the call ends with one copy and one wait,
 * without them it only enqueues.
 * RSDSFM_ERR_INVALID ("denoise temporal video: ..."): rsdsfm_denoise_video_dev's list and the frame call's. */
int rsdsfm_denoise_temporal_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                                      double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                                      const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                                      const rsdsfm_denoise_params* params_or_null, const rsdsfm_noise_curve_params* curve_or_null,
                                      const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images,
                                      uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null, uint8_t* const* d_out_supports_or_null, int64_t* counts_or_null,
                                      uint64_t* noise_curves_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_NOISE_TEMPORAL_H */
