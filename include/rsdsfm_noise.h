/*
 * rsdsfm_noise.h -- C ABI of the noise level on the MI355X: one frame's noise, measured from the frame itself, and the temporal denoise and
 * the spatial top-up (rsdsfm_denoise.h, which this header includes) with their strength h formed from it ON THE DEVICE: no host wait stands
 * between the measurement and its use, as the accumulate already forms its gains from the blend's 8-word record.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523), never looks at a frame's noise and has no
 * counterpart to this.  The denoise's fixed default h = 12 suits the one noise level it was tried at (+-6); at +-20 it hardly denoises, and at
 * +-2 it is wider than it has to be, which costs nothing on a static scene but lets movers ghost.  tests/noise_spec_numpy.py is the executable
 * definition; every call here reproduces it bit for bit.  Integers only.
 *   mask K      [[1, -2, 1], [-2, 4, -2], [1, -2, 1]] (Immerkaer): it annihilates constant, linear and xy terms; sum K^2 = 36.
 *   candidates  pixel p with 1 <= y <= rows - 2, 1 <= x <= cols - 2 whose nine mask bytes (its 3 x 3 window) are all non-zero.
 *   samples     channel c of a candidate whose nine bytes all lie in 1 .. 254 (a clipped byte carries no noise).  r = sum K I_c, |r| <= 2024.
 *   histogram   hist[min(|r|, 1023)] += 1: 1024 uint32 bins, all channels pooled; at most 3 * 16384^2 < 2^32 samples.
 *   record      four uint64 [n, m, sigma_q8, 0]: n = sum hist; k = max(1, (n q + 255) >> 8), q = quantile_q8 in 1 .. 256 (0: 128, the median);
 *               m = the smallest bin whose cumulative count is >= k, 0 when n == 0; sigma_q8 = (256000 m + 2023) / 4047: sigma in 1 / 256 grey
 *               levels (r has standard deviation 6 sigma, the median of |N(0, 1)| is 0.6745: median |r| = 4.047 sigma).
 *   strength    fallback where n < min_samples, else clamp((scale m + 8) >> 4, 1, 255).  scale = 12 gives h = 12 at m = 16, what the project's
 *               quality scene measures at +-6: h = 3.04 sigma.  At m >= 340 h is 255: clamping the bins at 1023 loses nothing.
 * The quantile's default (the median) and min_samples' default (1024, the blend's min_overlap) are choices, not measurements; scale's default is
 * derived from the existing default strength as above.  DESIGN.md section 12 ("Noise level") has the kernels, the LDS layout, the contention
 * argument and the bytes.
 *
 * NOT here: the same for the super-resolution and the sharpness transfer, signal-dependent (Poisson) noise, a sigma per channel or per region, a
 * temporal estimator from registered differences, the fuzz campaign entry, the C++ mirror.
 */
#ifndef RSDSFM_NOISE_H
#define RSDSFM_NOISE_H

#include "rsdsfm_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSDSFM_NOISE_BINS 1024
#define RSDSFM_NOISE_QUANTILE_MAX 256
/* the defaults: the quantile and min_samples are choices, not measurements; the scale is derived (see above) */
#define RSDSFM_NOISE_QUANTILE_DEFAULT 128
#define RSDSFM_NOISE_SCALE_DEFAULT 12
#define RSDSFM_NOISE_MIN_SAMPLES_DEFAULT 1024

typedef struct rsdsfm_noise_params {
    int32_t quantile_q8;  /* q, 1 .. 256; 0: the default, 128 (the median) */
    int32_t scale;        /* h = (scale m + 8) >> 4, 1 .. 255; 0: the default, 12 */
    int32_t struct_bytes; /* 0 or sizeof(rsdsfm_noise_params), as rsdsfm_noise_params_init sets it; anything else is refused */
    int32_t reserved0;    /* 0 */
    int64_t min_samples;  /* samples below which the strength is the fallback, >= 0; 0: the default, 1024 */
    int32_t reserved[4];  /* 0 */
} rsdsfm_noise_params;

/* quantile_q8 = 128, scale = 12, min_samples = 1024, struct_bytes = sizeof.  A NULL params pointer means these values. */
int rsdsfm_noise_params_init(rsdsfm_noise_params* params);

/* The histogram and the record as defined above.  d_image: rows x cols x channels bytes, channels 1 or 3; d_mask: rows x cols bytes; DEVICE,
 * 4-byte aligned, only read.  quantile_q8 0 .. 256, 0 meaning 128.  d_hist1024_out: 1024 uint32 on the DEVICE, 4-byte aligned; d_record4_out:
 * four uint64 on the DEVICE, 8-byte aligned; every word of both is written, so they need no preset; distinct from the inputs and from each
 * other.  rows, cols in [2, 16384]; a 2-row or 2-column image has no candidate: n = 0.
 * Enqueues one memset (the histogram) and two launches on the context's stream -- noise_hist_kernel<CH>, one 32-bit integer atomicAdd per
 * non-zero bin and workgroup, and noise_resolve_kernel, one workgroup -- and returns without waiting.  Integer sums: exact and independent of
 * scheduling.
 * RSDSFM_ERR_INVALID with a "noise level: ..." message and nothing enqueued: a NULL, misaligned or aliased pointer, channels, a size or the
 * quantile outside its range. */
int rsdsfm_noise_level_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols, int32_t quantile_q8,
                           uint32_t* d_hist1024_out, uint64_t* d_record4_out);

/* Kernel launches of rsdsfm_noise_level_dev: 2.  The memset of the histogram is not counted.  Host only. */
int rsdsfm_noise_level_launches(void);

/* The strength as defined above, on the host: what the auto calls form on the device.  n, m: the record's first two words; scale 0 .. 255 (0:
 * 12); fallback 1 .. 255 (0: 12, the denoise's default); min_samples >= 0 (0: 1024).  Returns h in 1 .. 255, or RSDSFM_ERR_INVALID (negative)
 * for n < 0, m < 0 or a parameter outside its range.  Host only. */
int rsdsfm_noise_strength(int64_t n, int64_t m, int32_t scale, int32_t fallback, int64_t min_samples);

/* rsdsfm_denoise_accumulate_dev with the strength from a record: its arguments, with d_noise4 (four uint64 on the DEVICE, 8-byte aligned, only
 * read: rsdsfm_noise_level_dev's record), scale and min_samples behind `strength`, which becomes the fallback.  Every workgroup loads n and m
 * and forms h itself.  Every byte is the existing call's made with strength = rsdsfm_noise_strength(n, m, scale, strength, min_samples).  One
 * kernel launch (denoise_accumulate_auto_kernel<CH, FIRST, LAST>).
 * RSDSFM_ERR_INVALID ("denoise auto accumulate: ...", "denoise auto: ..."): the existing call's list, a NULL, misaligned or aliased d_noise4,
 * scale outside [0, 255], min_samples < 0. */
int rsdsfm_denoise_accumulate_auto_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image_or_null,
                                       const uint8_t* d_layer_mask_or_null, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                                       int64_t min_overlap, int32_t gain_mode, int32_t strength, const uint64_t* d_noise4, int32_t scale, int64_t min_samples,
                                       uint16_t* d_cells_or_null, int32_t first, int32_t last, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null,
                                       int64_t* d_counts3_or_null);

/* rsdsfm_denoise_spatial_dev with the strength from a record, in the same way (denoise_spatial_auto_kernel<CH, S>).
 * RSDSFM_ERR_INVALID ("denoise spatial auto: ..."): the existing call's list, a NULL, misaligned or aliased d_noise4, scale, min_samples. */
int rsdsfm_denoise_spatial_auto_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, const uint8_t* d_weight_or_null, int32_t channels, int32_t rows,
                                    int32_t cols, int32_t strength, const uint64_t* d_noise4, int32_t scale, int64_t min_samples, int32_t target, int32_t search,
                                    uint8_t* d_image_out, uint8_t* d_support_or_null, int64_t* d_counts3_or_null);

/* One frame denoised at the strength its own noise asks for: rsdsfm_denoise_frame_dev's arguments and order, with three differences.
 *   1. Right after the own render rsdsfm_noise_level_dev measures the rendered reference planes (R, mR) with noise->quantile_q8.  Measuring
 *      BEHIND the bilinear render is deliberate: the render smooths, and R's noise is the noise the weight formula compares.
 *   2. Every neighbour step is rsdsfm_denoise_accumulate_auto_dev on that record (params->strength is the fallback).
 *   3. With spatial_or_null the temporal result goes to planes of the context's workspace, as in rsdsfm_denoise_spatial_frame_dev, and
 *      rsdsfm_denoise_spatial_auto_dev follows on the same record (spatial->strength is the fallback) into d_image_out and d_support_or_null.
 * d_counts6_or_null: six DEVICE int64 [unset, own only, averaged, unset, kept, smoothed], 8-byte aligned; without the top-up words 3 .. 5 are
 * zeroed.  d_support_or_null needs spatial_or_null.  d_noise4_or_null: four DEVICE uint64, 8-byte aligned: the frame's record [n, m, sigma_q8,
 * 0], none of the outputs and none of the sources' images, depth maps and pose tables; NULL: the record stays in the workspace.  The histogram (4 KB) and a record join the dense workspace with the first call and are
 * released by rsdsfm_destroy: a context that never asks keeps its footprint.  With nsrc == 1 the record is measured and the single accumulate
 * has no layer to weigh.  Every output is byte for byte the public calls made one after another; whatever any of them would refuse is refused
 * before the first enqueues.  Returns without waiting.
 * RSDSFM_ERR_INVALID ("denoise auto frame: ..."): rsdsfm_denoise_frame_dev's and rsdsfm_denoise_spatial_frame_dev's lists, the noise
 * parameters, a support plane without the top-up, a misaligned or aliased d_noise4_or_null, bad struct_bytes. */
int rsdsfm_denoise_auto_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                                  const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                                  int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_denoise_params* params_or_null,
                                  const rsdsfm_noise_params* noise_or_null, const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null,
                                  uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, uint8_t* d_support_or_null, int64_t* d_counts6_or_null,
                                  uint64_t* d_noise4_or_null);

/* = rsdsfm_denoise_launches(rows, cols, nsrc) + 2, + 1 more with the top-up (with_spatial != 0), and its refusals.  Host only. */
int rsdsfm_denoise_auto_frame_launches(int32_t rows, int32_t cols, int32_t nsrc, int32_t with_spatial);

/* rsdsfm_denoise_video_dev with rsdsfm_denoise_auto_frame_dev per frame: the same clip, walk and neighbours, into d_out_images[q],
 * d_out_masks[q], d_out_weights_or_null[q] and d_out_supports_or_null[q] (either array may be NULL; the supports need spatial_or_null).
 * counts_or_null: HOST, nsources x 6 int64; noise_records_or_null: HOST, nsources x 4 uint64, every frame's record.  With either the call ends
 * with one copy and one wait, without them it only enqueues.
 * RSDSFM_ERR_INVALID ("denoise auto video: ..."): rsdsfm_denoise_video_dev's list and the frame call's. */
int rsdsfm_denoise_auto_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                                  double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                                  const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                                  const rsdsfm_denoise_params* params_or_null, const rsdsfm_noise_params* noise_or_null,
                                  const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images,
                                  uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null, uint8_t* const* d_out_supports_or_null, int64_t* counts_or_null,
                                  uint64_t* noise_records_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_NOISE_H */
