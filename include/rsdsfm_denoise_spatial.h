/*
 * rsdsfm_denoise_spatial.h -- C ABI of the spatial top-up on the MI355X, the single-frame denoiser beside the temporal denoise (rsdsfm_denoise.h,
 * which includes this header at its end: either include gives both): a patch-weighted mean of a pixel's neighbours in its OWN frame, mixed
 * with the pixel in proportion to what the temporal stage did not give it.  The stage writes what this needs, the weight plane n; with no
 * weight plane the call denoises any 8-bit image under a mask, the dense rectifier's output included.  tests/denoise_spatial_spec_numpy.py is the executable definition; every call reproduces it bit for bit.
 *   inputs      image I (rows x cols x channels bytes, channels 1 or 3), mask m (v(p): m(p) is not 0), optional weight plane n (bytes; absent:
 *               n(p) = 16 where v(p)).
 *   candidates  q = p + d, d in [-S, S]^2 without 0, q inside the frame, v(p) and v(q).
 *   patch       over the o in {-1, 0, 1}^2 with p + o and q + o inside the frame and both set: D = sum_o sum_c |I_c(p + o) - I_c(q + o)|,
 *               N = channels #{o}; w_q = 16 - min(16, (16 D) / (h N)) in integer division: the temporal formula between two places of one image.
 *               Sw = sum_q w_q, s_c = sum_q w_q I_c(q).
 *   top-up      delta = max(0, target - n(p)); B = max(128, Sw); W = n(p) B + delta Sw.  Where v(p) and W > 0
 *               out_c = (2 (n B I_c(p) + delta s_c) + W) / (2 W) (round half up); where v(p) and W == 0 (only n = 0) out_c = I_c(p); where not
 *               v(p) out_c = 0.  The mask is the input's.  128 is eight full-weight candidates, all of S = 1: a wider search only adds support.
 *   support     min(255, (2 W + B) / (2 B)) where v(p), else 0.
 *   counters    [unset: not v(p); kept: v(p) and delta Sw == 0, the output is I(p) byte for byte; smoothed: the rest].
 * Nothing overflows 32 bits (n B I <= 255 * 768 * 255, delta s_c likewise).  A pixel with n >= target keeps its bytes exactly.
 * The defaults (strength 12: the temporal default; target 80 = 16 (1 + 2 * 2): a fully supported pixel at the temporal default radius; search
 * 2) are choices, not measurements.  DESIGN.md section 12 ("Spatial top-up") has the kernel, the LDS layout and the bytes.
 *
 * NOT here: search windows beyond 7 x 7, patches other than 3 x 3, a noise-level estimate (built since: rsdsfm_noise.h), the same top-up for super-resolution and sharpness
 * transfer, the fuzz campaign entry, the C++ mirror.
 */
#ifndef RSDSFM_DENOISE_SPATIAL_H
#define RSDSFM_DENOISE_SPATIAL_H

#include "rsdsfm_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSDSFM_DENOISE_SPATIAL_SEARCH_MAX 3
/* the defaults: choices, not measurements */
#define RSDSFM_DENOISE_SPATIAL_TARGET_DEFAULT 80
#define RSDSFM_DENOISE_SPATIAL_SEARCH_DEFAULT 2

typedef struct rsdsfm_denoise_spatial_params {
    int32_t strength;     /* h, 1 .. 255; 0: the default, 12 */
    int32_t target;       /* the weight at which a pixel is left alone, 1 .. 255; 0: the default, 80 */
    int32_t search;       /* S: candidates within [-S, S]^2, 1 .. 3; 0: the default, 2 */
    int32_t struct_bytes; /* 0 or sizeof(rsdsfm_denoise_spatial_params), as rsdsfm_denoise_spatial_params_init sets it; anything else is refused */
    int32_t reserved[4];  /* 0 */
} rsdsfm_denoise_spatial_params;

/* strength = 12, target = 80, search = 2, struct_bytes = sizeof.  A NULL params pointer means these values. */
int rsdsfm_denoise_spatial_params_init(rsdsfm_denoise_spatial_params* params);

/* The top-up as defined above.  d_image: rows x cols x channels bytes; d_mask, d_weight_or_null: rows x cols bytes; DEVICE, only read.
 * strength, target 0 .. 255 and search 0 .. 3, 0 meaning the default.  d_image_out (rows x cols x channels bytes) and d_support_or_null (rows x
 * cols bytes): every byte is written, so they need no preset.  d_counts3_or_null: a DEVICE array [unset, kept, smoothed] of three int64, 8-byte
 * aligned; the call zeroes it (a memset on the context's stream, a stream node of its own) and the kernel adds to it as the accumulate does.
 * Every plane is 4-byte aligned; the outputs are distinct from the inputs and from each other; rows, cols in [2, 16384].
 * One kernel launch (denoise_spatial_kernel<CH, S>) on the context's stream; returns without waiting.  A workgroup none of whose pixels is set
 * and below the target copies its pixels: a frame the temporal stage fully supported costs a copy.
 * RSDSFM_ERR_INVALID with a "denoise spatial: ..." message and nothing enqueued: a NULL, misaligned or aliased pointer, channels, a size, strength,
 * target or search outside its range. */
int rsdsfm_denoise_spatial_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, const uint8_t* d_weight_or_null, int32_t channels, int32_t rows,
                               int32_t cols, int32_t strength, int32_t target, int32_t search, uint8_t* d_image_out, uint8_t* d_support_or_null,
                               int64_t* d_counts3_or_null);

/* Kernel launches of rsdsfm_denoise_spatial_dev: 1.  The memset of the counters is not counted.  Host only. */
int rsdsfm_denoise_spatial_launches(void);

/* One frame through the temporal denoise and the top-up: rsdsfm_denoise_frame_dev (its arguments and params_or_null) into planes of the context's
 * dense workspace -- the image, and the weight when d_weight_or_null is NULL (CH + 1 bytes per pixel, joined with the first call, released with
 * the rest) --, d_mask_out, the caller's weight plane and counters 0 .. 2, then rsdsfm_denoise_spatial_dev (spatial_or_null) from those planes into
 * d_image_out, d_support_or_null and counters 3 .. 5.  d_counts6_or_null: six DEVICE int64 [unset, own only, averaged, unset, kept, smoothed],
 * 8-byte aligned.  Byte for byte the two public calls one after another; no host wait.
 * RSDSFM_ERR_INVALID ("denoise spatial frame: ..."): the frame call's list, the spatial parameters, bad struct_bytes. */
int rsdsfm_denoise_spatial_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                                     const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows,
                                     int32_t cols, int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m,
                                     const rsdsfm_denoise_params* params_or_null, const rsdsfm_denoise_spatial_params* spatial_or_null, const int32_t* window_or_null,
                                     uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, uint8_t* d_support_or_null, int64_t* d_counts6_or_null);

/* = rsdsfm_denoise_launches(rows, cols, nsrc) + 1, and its refusals.  Host only. */
int rsdsfm_denoise_spatial_frame_launches(int32_t rows, int32_t cols, int32_t nsrc);

/* rsdsfm_denoise_video_dev with the top-up behind every frame: the same clip, walk and neighbours, rsdsfm_denoise_spatial_frame_dev per frame into
 * d_out_images[q], d_out_masks[q], d_out_weights_or_null[q] and d_out_supports_or_null[q] (either array may be NULL).  counts_or_null: HOST,
 * nsources x 6 int64; with it the call ends with one copy and one wait, without it the call only enqueues.
 * RSDSFM_ERR_INVALID ("denoise spatial video: ..."): rsdsfm_denoise_video_dev's list and the frame call's. */
int rsdsfm_denoise_spatial_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx,
                                     double fy, double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t,
                                     const double* A, const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode,
                                     int32_t iterations, const rsdsfm_denoise_params* params_or_null, const rsdsfm_denoise_spatial_params* spatial_or_null,
                                     const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null,
                                     uint8_t* const* d_out_supports_or_null, int64_t* counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_DENOISE_SPATIAL_H */
