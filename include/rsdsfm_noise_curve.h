/*
 * rsdsfm_noise_curve.h -- C ABI of the noise curve on the MI355X: one frame's noise measured PER BRIGHTNESS LEVEL from the frame itself, and the
 * temporal denoise and the spatial top-up (rsdsfm_noise.h, which this header includes) with a strength h PER PIXEL formed from it ON THE DEVICE.
 *
 * rsdsfm_noise.h measures ONE number per frame.  A sensor's noise is signal-dependent (shot noise: sigma^2 roughly a L + b), so that one h is too
 * wide in the shadows, where movers then ghost, and too narrow in the highlights, which stay noisy.  The reference has no counterpart.
 * tests/noise_curve_spec_numpy.py is the executable definition; every call here reproduces it bit for bit.  Integers only.
 *   samples     the candidates, the samples and r = sum K I_c exactly as in rsdsfm_noise.h.
 *   level       of the sample (p, c): S = the sum of channel c's nine bytes about p, L = (S + 4) / 9, in 1 .. 254.  Band b = L >> 5.
 *   histogram   hist[b][min(|r|, 1023)] += 1: 8 x 1024 uint32 (32 KB).  The eight bands sum to rsdsfm_noise_level_dev's histogram.
 *   curve       36 uint64, nine rows [n, m, sigma_q8, 0]: rows 0 .. 7 rsdsfm_noise.h's record of each band's histogram, row 8 the record of
 *               their sum: rsdsfm_noise_level_dev's record.
 *   strengths   256 bytes h(L).  Row 8 with n < min_samples: every entry is the fallback.  Band b is valid iff n_b >= band_min_samples.
 *               mfill_b = m_b of a valid band, else the m of the nearest valid band (the lower one on a tie), row 8's m when none is valid.
 *               The band centres are 32 b + 16.  L < 16: M32 = 32 mfill_0; L >= 240: M32 = 32 mfill_7; else b = (L - 16) >> 5,
 *               t = (L - 16) & 31, M32 = (32 - t) mfill_b + t mfill_{b + 1}: linear between centres, so that no band border shows.
 *               h(L) = clamp((scale M32 + 256) >> 9, 1, 255).  A flat curve (every mfill = m) gives rsdsfm_noise_strength's (scale m + 8) >> 4.
 *   consumers   a pixel's level is its byte (gray) or (b + g + r + 1) / 3 (BGR): of the REFERENCE pixel in the accumulate, of the centre pixel
 *               in the top-up.  The weight formulas are the existing ones with `strength` replaced by h(level).
 * band_min_samples' default (256) is a choice, not a measurement; the other defaults are rsdsfm_noise.h's.  DESIGN.md section 12 ("Noise
 * curve") has the kernels, the LDS layout and the bytes.
 *
 * NOT here: the curve for the super-resolution and the sharpness transfer, a sigma per channel, a fitted a L + b model in place of eight
 * medians, monotonicity enforcement, the fuzz campaign entry, the C++ mirror.
 */
#ifndef RSDSFM_NOISE_CURVE_H
#define RSDSFM_NOISE_CURVE_H

#include "rsdsfm_noise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSDSFM_NOISE_CURVE_BANDS 8
#define RSDSFM_NOISE_CURVE_ROWS 9
#define RSDSFM_NOISE_CURVE_WORDS 36
#define RSDSFM_NOISE_CURVE_HIST_WORDS (RSDSFM_NOISE_CURVE_BANDS * RSDSFM_NOISE_BINS)
/* a choice, not a measurement */
#define RSDSFM_NOISE_CURVE_BAND_MIN_SAMPLES_DEFAULT 256

typedef struct rsdsfm_noise_curve_params {
    int32_t quantile_q8;      /* q, 1 .. 256; 0: the default, 128 (the median) */
    int32_t scale;            /* 1 .. 255; 0: the default, 12 */
    int32_t struct_bytes;     /* 0 or sizeof(rsdsfm_noise_curve_params), as rsdsfm_noise_curve_params_init sets it; anything else is refused */
    int32_t reserved0;        /* 0 */
    int64_t min_samples;      /* row 8's samples below which every strength is the fallback, >= 0; 0: the default, 1024 */
    int64_t band_min_samples; /* a band's samples below which its m is taken from its nearest valid neighbour, >= 0; 0: the default, 256 */
    int32_t reserved[4];      /* 0 */
} rsdsfm_noise_curve_params;

/* quantile_q8 = 128, scale = 12, min_samples = 1024, band_min_samples = 256, struct_bytes = sizeof.  A NULL params pointer means these values. */
int rsdsfm_noise_curve_params_init(rsdsfm_noise_curve_params* params);

/* The banded histogram and the curve as defined above.  d_image, d_mask, channels, rows, cols, quantile_q8: as rsdsfm_noise_level_dev takes
 * them.  d_hist8192_out: 8 x 1024 uint32 on the DEVICE, 4-byte aligned; d_curve36_out: 36 uint64 on the DEVICE, 8-byte aligned; every word of
 * both is written, so they need no preset; distinct from the inputs and from each other.  rows, cols in [2, 16384].
 * Enqueues one memset (the 32 KB histogram) and two launches on the context's stream -- noise_curve_hist_kernel<CH>, one 32-bit integer
 * atomicAdd per non-zero bin and workgroup, and noise_curve_resolve_kernel, nine independent workgroups -- and returns without waiting.
 * Integer sums: exact and independent of scheduling.
 * RSDSFM_ERR_INVALID with a "noise curve: ..." message and nothing enqueued: a NULL, misaligned or aliased pointer, channels, a size or the
 * quantile outside its range. */
int rsdsfm_noise_curve_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols, int32_t quantile_q8,
                           uint32_t* d_hist8192_out, uint64_t* d_curve36_out);

/* Kernel launches of rsdsfm_noise_curve_dev: 2.  The memset of the histogram is not counted.  Host only. */
int rsdsfm_noise_curve_launches(void);

/* The strength table as defined above, on the host: exactly what the consumers form on the device.  curve36: 36 HOST uint64; scale 0 .. 255
 * (0: 12); fallback 0 .. 255 (0: 12, the denoise's default); min_samples >= 0 (0: 1024); band_min_samples >= 0 (0: 256); lut256_out: 256 HOST
 * bytes.  Returns RSDSFM_OK, or RSDSFM_ERR_INVALID for a NULL pointer or a parameter outside its range.  Host only. */
int rsdsfm_noise_curve_strengths(const uint64_t* curve36, int32_t scale, int32_t fallback, int64_t min_samples, int64_t band_min_samples, uint8_t* lut256_out);

/* rsdsfm_denoise_accumulate_auto_dev with the strength per pixel from a curve: its arguments, with d_curve36 (36 uint64 on the DEVICE, 8-byte
 * aligned, only read: rsdsfm_noise_curve_dev's curve) in the record's place and band_min_samples behind min_samples; `strength` is the
 * fallback.  Every workgroup forms the 256-entry table in LDS itself; a pixel's strength is the entry at the level of the REFERENCE pixel.
 * With row 8 below min_samples every byte is the existing call's at the fallback; with a flat curve every byte is the existing call's at
 * rsdsfm_noise_strength(n, m, scale, strength, min_samples).  One kernel launch (denoise_accumulate_curve_kernel<CH, FIRST, LAST>).
 * RSDSFM_ERR_INVALID ("denoise curve accumulate: ...", "denoise curve: ..."): the existing call's list, a NULL, misaligned or aliased
 * d_curve36, scale outside [0, 255], min_samples < 0, band_min_samples < 0. */
int rsdsfm_denoise_accumulate_curve_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image_or_null,
                                        const uint8_t* d_layer_mask_or_null, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                                        int64_t min_overlap, int32_t gain_mode, int32_t strength, const uint64_t* d_curve36, int32_t scale, int64_t min_samples,
                                        int64_t band_min_samples, uint16_t* d_cells_or_null, int32_t first, int32_t last, uint8_t* d_image_out, uint8_t* d_mask_out,
                                        uint8_t* d_weight_or_null, int64_t* d_counts3_or_null);

/* rsdsfm_denoise_spatial_auto_dev with the strength per pixel from a curve, in the same way: the entry at the level of the centre pixel
 * (denoise_spatial_curve_kernel<CH, S>).
 * RSDSFM_ERR_INVALID ("denoise curve spatial: ..."): the existing call's list, a NULL, misaligned or aliased d_curve36, scale, min_samples,
 * band_min_samples. */
int rsdsfm_denoise_spatial_curve_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, const uint8_t* d_weight_or_null, int32_t channels, int32_t rows,
                                     int32_t cols, int32_t strength, const uint64_t* d_curve36, int32_t scale, int64_t min_samples, int64_t band_min_samples,
                                     int32_t target, int32_t search, uint8_t* d_image_out, uint8_t* d_support_or_null, int64_t* d_counts3_or_null);

/* rsdsfm_denoise_auto_frame_dev with the curve in the record's place: right after the own render rsdsfm_noise_curve_dev measures the rendered
 * reference planes with curve->quantile_q8, every neighbour step is rsdsfm_denoise_accumulate_curve_dev on that curve (params->strength is the
 * fallback), and with spatial_or_null rsdsfm_denoise_spatial_curve_dev follows on the same curve (spatial->strength is the fallback).
 * d_curve36_or_null: 36 DEVICE uint64, 8-byte aligned: the frame's curve, none of the outputs and none of the sources' images, depth maps and
 * pose tables; NULL: the curve stays in the workspace.  The histogram (32 KB) and a curve join the dense workspace with the first call and are
 * released by rsdsfm_destroy: a context that never asks keeps its footprint.  Every output is byte for byte the public calls made one after
 * another; whatever any of them would refuse is refused before the first enqueue.  Returns without waiting.
 * RSDSFM_ERR_INVALID ("denoise curve frame: ..."): rsdsfm_denoise_auto_frame_dev's list with the curve's parameters in the noise parameters'
 * place. */
int rsdsfm_denoise_curve_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                                   const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                                   int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_denoise_params* params_or_null,
                                   const rsdsfm_noise_curve_params* curve_or_null, const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null,
                                   uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, uint8_t* d_support_or_null, int64_t* d_counts6_or_null,
                                   uint64_t* d_curve36_or_null);

/* = rsdsfm_denoise_launches(rows, cols, nsrc) + 2, + 1 more with the top-up (with_spatial != 0), and its refusals.  Host only. */
int rsdsfm_denoise_curve_frame_launches(int32_t rows, int32_t cols, int32_t nsrc, int32_t with_spatial);

/* rsdsfm_denoise_auto_video_dev with rsdsfm_denoise_curve_frame_dev per frame.  counts_or_null: HOST, nsources x 6 int64;
 * noise_curves_or_null: HOST, nsources x 36 uint64, every frame's curve.  With either the call ends with one copy and one wait, without them
 * it only enqueues.
 * RSDSFM_ERR_INVALID ("denoise curve video: ..."): rsdsfm_denoise_video_dev's list and the frame call's. */
int rsdsfm_denoise_curve_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                                   double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                                   const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                                   const rsdsfm_denoise_params* params_or_null, const rsdsfm_noise_curve_params* curve_or_null,
                                   const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images,
                                   uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null, uint8_t* const* d_out_supports_or_null, int64_t* counts_or_null,
                                   uint64_t* noise_curves_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_NOISE_CURVE_H */
