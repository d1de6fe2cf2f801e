/*
 * rsdsfm_shutter.h -- C ABI of the synthetic shutter on the MI355X: a frame of a solved clip EXPOSED over a window of time about an instant, the
 * mean of the scene rendered at S sub-instants along the camera path -- motion blur from sub-instant renders.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  Every
 * frame of rsdsfm_retime.h is an instantaneous view, which suits slow motion; a 60 -> 24 fps conversion, or constant pacing from irregular
 * input, strobes when every output frame has a zero-length exposure.  The shutter is the temporal integrator behind the retimer:
 *   sub-instants  (host, double) for an instant t, a width `shutter` in units of input-frame intervals and S = samples:
 *                 u_j = (j + 0.5) / S - 0.5, t_j = t + shutter * u_j, j = 0 .. S - 1, evaluated exactly in this order.  t_j is KEPT iff
 *                 0 <= t_j <= nsources - 1: an exposure window is clipped at the clip's ends.  S = 1 gives t_0 == t bitwise, shutter = 0 makes
 *                 every t_j == t; at least one sub-instant is always kept.
 *   cell          per pixel, BGR: four uint16 [s_b, s_g, s_r, n] (8 B); gray: two uint16 [s, n] (4 B).  64 * 255 = 16 320: nothing overflows.
 *   accumulate    one sample (image, mask) with the flags first and last; a pixel of the sample counts iff its mask byte != 0:
 *                 first      every cell is the sample's pixel and n = 1, or all 0 where the mask is 0; what the cells held never shows
 *                 not first  s_c += v_c and n += 1 where the mask is set
 *                 not last   the cells are written (where a four-pixel mask word is 0 and first is off they are neither read nor written)
 *                 last       the cells are NOT written; the frame is resolved: where n >= min_samples out_c = (2 s_c + n) / (2 n) in integer
 *                            division (the mean, round half up) and mask 1, else image 0 and mask 0 (left to the fill and the inpainter);
 *                            coverage = n; the counters [unset: n < min_samples, partial: min_samples <= n < nsamples, full: n == nsamples]
 *                 The sums are integers: the result does not depend on the order of the samples.
 *   frame         for every kept sub-instant in order rsdsfm_retime_poses(t_j), rsdsfm_retime_frame_dev into a sample image and mask of the
 *                 context's workspace, and the accumulate call (first on the first kept one, last on the last) with nsamples = the KEPT count
 *                 and min_samples = min(params.min_samples, kept): a window clipped at the clip's end asks of a pixel what it can give.
 * Integers only on the device; tests/shutter_spec_numpy.py is the executable definition and every call here reproduces it bit for bit.
 * DESIGN.md section 12 ("Synthetic shutter") has the kernel, the bytes, the launches and what has been measured.
 *
 * NOT here: weighted (non-box) shutters, a fused render-and-accumulate kernel that skips the sample planes, rolling-shutter re-synthesis, fill
 * or inpaint of the exposed frame (the generic frame calls rsdsfm_stabilize_window_frame_dev, rsdsfm_seam_blend_layer_dev and
 * rsdsfm_inpaint_frame_dev accept this header's outputs), the C++ mirror.
 */
#ifndef RSDSFM_SHUTTER_H
#define RSDSFM_SHUTTER_H

#include "rsdsfm_retime.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSDSFM_SHUTTER_SAMPLES_MAX 64
/* the defaults: choices, not measurements (0.5 is the 180 degree shutter of a clip retimed at factor 1) */
#define RSDSFM_SHUTTER_DEFAULT 0.5
#define RSDSFM_SHUTTER_SAMPLES_DEFAULT 8
#define RSDSFM_SHUTTER_MIN_SAMPLES_DEFAULT 1

typedef struct rsdsfm_shutter_params {
    double shutter;       /* the exposure window's width in input-frame intervals, finite, 0 .. nsources - 1; 0: every sub-instant is t itself */
    int32_t samples;      /* S, 1 .. 64 */
    int32_t min_samples;  /* 1 .. samples: a pixel fewer kept sub-instants saw is left unset */
    int32_t struct_bytes; /* 0 or sizeof(rsdsfm_shutter_params), as rsdsfm_shutter_params_init sets it; anything else is refused */
    int32_t reserved[3];  /* 0 */
} rsdsfm_shutter_params;

/* shutter = 0.5, samples = 8, min_samples = 1, struct_bytes = sizeof.  A NULL params pointer means these values. */
int rsdsfm_shutter_params_init(rsdsfm_shutter_params* params);

/* HOST only, double, no context: the kept sub-instants of the exposure about t, in order, into times_out[0 .. *nkept_out - 1] (room for
 * `samples` doubles; the entries behind the kept ones are not written).  nsources: as rsdsfm_retime_poses takes it.
 * RSDSFM_ERR_INVALID: a NULL pointer, samples outside [1, 64], nsources < 1, shutter not finite, < 0 or > nsources - 1, t not finite or
 * outside [0, nsources - 1] (what rsdsfm_retime_poses refuses). */
int rsdsfm_shutter_times(double t, double shutter, int32_t samples, int32_t nsources, double* times_out, int32_t* nkept_out);

/* One sample accumulated, as defined above.  d_image (rows x cols x channels bytes, channels 1 or 3) and d_mask (rows x cols bytes, 0 = empty,
 * anything else set): DEVICE, only read.  d_cells_or_null: rows x cols cells, DEVICE, 8-byte aligned; it may be NULL only with first && last.
 * first, last: 0 or 1.  nsamples 1 .. 64 (what "full" means), min_samples 1 .. nsamples; both are read only when last.
 * d_image_out, d_mask_out, d_coverage_or_null (rows x cols bytes), d_counts3_or_null are read only when last, and then every byte of the output
 * planes is written, so they need no preset.  d_counts3_or_null: a DEVICE array [unset, partial, full] of three int64, 8-byte aligned; the call
 * zeroes it (a memset on the context's stream) and the kernel adds to it -- a sum per workgroup with shuffles and LDS, then three 64-bit
 * integer atomics per workgroup: exact and independent of scheduling.
 * Every plane is 4-byte aligned; the outputs are distinct from the inputs, from the cells and from each other, the cells from the inputs.
 * One kernel launch, enqueued on the context's stream; returns without waiting.  A refused call enqueues nothing.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased pointer, channels, a size outside [2, 16384], first or last other than 0 / 1, nsamples or
 * min_samples outside its range. */
int rsdsfm_shutter_accumulate_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols,
                                  uint16_t* d_cells_or_null, int32_t first, int32_t last, int32_t nsamples, int32_t min_samples, uint8_t* d_image_out,
                                  uint8_t* d_mask_out, uint8_t* d_coverage_or_null, int64_t* d_counts3_or_null);

/* Kernel launches of rsdsfm_shutter_accumulate_dev: 1.  The memset of the counters is not counted.  Host only. */
int rsdsfm_shutter_accumulate_launches(void);

/* One exposed frame of a solved clip, as defined above.  The clip is rsdsfm_retime_video_dev's: d_frames, d_depth_maps, d_R, d_t (HOST arrays
 * of nsources DEVICE pointers), the HOST arrays A, c, the path A_path, c_path and scales, the camera, mode, q5_mode and iterations.
 * shutter_or_null, retime_or_null: NULL means the defaults; window_or_null: (r0, c0, h, w), NULL = the full frame.
 * All sub-instants and all poses are computed before anything is enqueued.  Then, on the context's stream, per kept sub-instant
 * rsdsfm_retime_frame_dev into the workspace's sample planes (no source plane, no counters) and rsdsfm_shutter_accumulate_dev: every output is
 * byte for byte those public calls made one after another.  shutter = 0 with any samples, and samples = 1, give rsdsfm_retime_frame_dev's image
 * bytes and its mask.  *nkept_or_null: HOST, the kept count.  The sample planes and the cells (12 B per pixel) join the context's dense workspace
 * with the first call and after a size change and are released by rsdsfm_destroy: a context that never asks keeps its footprint.  Returns
 * without waiting.
 * RSDSFM_ERR_INVALID: a NULL array or entry, a misaligned or aliased plane, what rsdsfm_shutter_times refuses, min_samples outside [1, samples],
 * bad struct_bytes, and the lists of rsdsfm_retime_poses, rsdsfm_retime_frame_dev and rsdsfm_shutter_accumulate_dev. */
int rsdsfm_shutter_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                             double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                             const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations, double t,
                             const rsdsfm_shutter_params* shutter_or_null, const rsdsfm_retime_params* retime_or_null, const int32_t* window_or_null,
                             uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_coverage_or_null, int64_t* d_counts3_or_null, int32_t* nkept_or_null);

/* A clip: one rsdsfm_shutter_frame_dev per entry of times, in order, into d_out_images[i], d_out_masks[i] and d_out_coverage_or_null[i] (the
 * array may be NULL).  Every instant's sub-instants and poses are computed first: a refused time enqueues nothing.
 * kept_out: HOST, ntimes int32, the kept count per instant.  counts_or_null: HOST, ntimes x 3 int64 [unset, partial, full]; with it the call ends
 * with one copy and one wait, without it the call only enqueues.
 * RSDSFM_ERR_INVALID: a NULL array or entry, ntimes < 1, and the frame call's list. */
int rsdsfm_shutter_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                             double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                             const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                             const double* times, int32_t ntimes, const rsdsfm_shutter_params* shutter_or_null, const rsdsfm_retime_params* retime_or_null,
                             const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks, uint8_t* const* d_out_coverage_or_null,
                             int32_t* kept_out, int64_t* counts_or_null);

/* Kernel launches of one exposed frame whose kept sub-instants are n_one_source integer instants and n_two_sources others:
 * n_one_source rsdsfm_retime_launches(rows, cols, 1) + n_two_sources rsdsfm_retime_launches(rows, cols, 2) + one accumulate per sample.
 * RSDSFM_ERR_INVALID for a size outside [2, 16384], a negative count, or a sum outside [1, 64].  Host only. */
int rsdsfm_shutter_launches(int32_t rows, int32_t cols, int32_t n_one_source, int32_t n_two_sources);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_SHUTTER_H */
