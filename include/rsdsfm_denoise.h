/*
 * rsdsfm_denoise.h -- C ABI of the temporal denoise on the MI355X: a frame of a solved clip averaged with its neighbours in time, every
 * neighbour rendered ALONE into the frame's own (virtual) camera through its depth map and rolling-shutter pose table, with a weight per pixel
 * and neighbour from the difference over a 3 x 3 patch.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  The
 * interior of every stabilised frame is a single warp of one noisy input frame; handheld low-light footage wants a multi-frame noise reducer
 * behind the stabiliser, and the clip pipeline already registers the neighbours in 3-D, with occlusion handling, not by 2-D flow.
 *   inputs      the reference (image R, mask mR: the own frame in the target camera) and one layer (image L, mask mL: a neighbour rendered
 *               alone) per step; a mask byte is set iff it is not 0, image bytes under an unset mask byte never show.
 *   gains       per channel G_c from the 8-word record [count, sum image_c, sum layer_c, 0 ...] as rsdsfm_seam_gains computes it (clamped to
 *               [16384, 262144]; 65536 with gain_mode == 1, count < min_overlap, sum layer_c == 0, or no record);
 *               k_c = min(255, (G_c L_c + 32768) >> 16).
 *   weight      v(p) = mR(p) set and mL(p) set; e(p) = sum_c |R_c(p) - k_c(p)| where v(p); D(p) = sum of e(p') and N(p) = channels #{p'} over
 *               the p' of the 3 x 3 window about p inside the frame with v(p'); w(p) = 16 - min(16, (16 D) / (h N)) in integer division where
 *               v(p), else 0.  h: the strength, 1 .. 255.
 *   cell        per pixel, BGR: four uint16 [s_b, s_g, s_r, n] (8 B); gray: two uint16 [s, n] (4 B): rsdsfm_shutter.h's layout.
 *               first      the cell is [16 R_c, 16] where mR is set and all 0 elsewhere (what it held never shows); then the layer is added
 *               every step s_c += w k_c, n += w
 *               not last   the cells are written
 *               last       the cells are NOT written; where n > 0 out_c = (2 s_c + n) / (2 n) (round half up) and mask 1, else image 0 and
 *                          mask 0; the weight plane is n; the counters [unset: n == 0, own only: n == 16, averaged: n > 16]
 *               With at most RSDSFM_DENOISE_LAYERS_MAX = 14 layers n <= 240 and s_c <= 61 200: nothing overflows.  THE CALLER OF
 *               rsdsfm_denoise_accumulate_dev KEEPS TO 14 LAYERS per `first`; the call cannot count them.
 *   frame       the own frame through rsdsfm_stabilize_window_frame_dev, every neighbour alone on a zeroed layer, the record by
 *               rsdsfm_seam_overlap_sums_dev, one accumulate per neighbour.
 * The sums are integers: the result does not depend on the order of the layers, and a layer that disagrees with the own frame everywhere
 * (w = 0) leaves the own frame's bytes exactly.  Integers only on the device; tests/denoise_spec_numpy.py is the executable definition and
 * every call here reproduces it bit for bit.  DESIGN.md section 12 ("Temporal denoise") has the kernel, the bytes, the launches and the LDS
 * layout.
 *
 * The spatial top-up (rsdsfm_denoise_spatial.h, which this header includes at its end) is the single-frame denoiser beside it:
 * it reads the weight plane n and tops every pixel up from its own frame in proportion to what time did not give.
 *
 * NOT here: spatial (single-frame) denoising (built since: rsdsfm_denoise_spatial.h), patches other than 3 x 3, a noise-level estimate (built since:
 * rsdsfm_noise.h measures it per frame and forms the strength from it on the device; in this header's calls the strength is the caller's), moving objects (they only fall back to the own pixel; rsdsfm_denoise_spatial.h tops them up), fill, blend or inpaint of the result (the generic frame calls rsdsfm_stabilize_window_frame_dev,
 * rsdsfm_seam_blend_layer_dev and rsdsfm_inpaint_frame_dev accept this header's outputs), a fused render-and-accumulate kernel that skips the
 * layer, the C++ mirror.
 */
#ifndef RSDSFM_DENOISE_H
#define RSDSFM_DENOISE_H

#include "rsdsfm_shutter.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSDSFM_DENOISE_RADIUS_MAX 7
#define RSDSFM_DENOISE_LAYERS_MAX 14
/* the defaults: choices, not measurements */
#define RSDSFM_DENOISE_RADIUS_DEFAULT 2
#define RSDSFM_DENOISE_STRENGTH_DEFAULT 12

typedef struct rsdsfm_denoise_params {
    int32_t radius;            /* neighbours on each side for the clip call, 1 .. 7; 0: the default, 2 */
    int32_t strength;          /* h, 1 .. 255; 0: the default, 12 */
    int32_t gain_mode;         /* 0: every neighbour gain-matched to the own frame on their overlap, the default; 1: off */
    int32_t occlusion;         /* 0: the neighbours through rsdsfm_stabilize_window_frame_dev; 1: through the occlusion test */
    int32_t occlusion_tol_q16; /* the occlusion test's tolerance, 1 .. 65536; 0: its default */
    int32_t struct_bytes;      /* 0 or sizeof(rsdsfm_denoise_params), as rsdsfm_denoise_params_init sets it; anything else is refused */
    int64_t min_overlap;       /* overlap pixels below which a neighbour gets no gain, >= 0; 0: the default, 1024 (the blend's) */
    int32_t reserved[4];       /* 0 */
} rsdsfm_denoise_params;

/* radius = 2, strength = 12, gain_mode = 0, occlusion = 0, occlusion_tol_q16 = 0, min_overlap = 1024, struct_bytes = sizeof.  A NULL params
 * pointer means these values. */
int rsdsfm_denoise_params_init(rsdsfm_denoise_params* params);

/* The seam blend's record as a call of its own: d_sums8_out (8 uint64 on the DEVICE, 8-byte aligned) = [count, sum image_c, sum layer_c, 0 ...]
 * over the pixels with d_source == 1 and d_layer_mask != 0 (rsdsfm_stabilize_blend.h).  d_image, d_layer: rows x cols x channels bytes;
 * d_source, d_layer_mask: rows x cols bytes; all DEVICE, 4-byte aligned, only read.  Enqueues one memset (the record) and the blend's sums
 * kernel on the context's stream -- what rsdsfm_seam_blend_layer_dev enqueues in front of its blend kernel -- and returns without waiting.
 * RSDSFM_ERR_INVALID: a NULL or misaligned pointer, channels other than 1 / 3, a size outside [2, 16384]. */
int rsdsfm_seam_overlap_sums_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_source, const uint8_t* d_layer, const uint8_t* d_layer_mask,
                                 int32_t channels, int32_t rows, int32_t cols, uint64_t* d_sums8_out);

/* One step, as defined above.  d_ref_image, d_layer_image_or_null: rows x cols x channels bytes, channels 1 or 3; d_ref_mask,
 * d_layer_mask_or_null: rows x cols bytes; DEVICE, only read.  The two layer pointers are both given or both NULL; NULL (no layer) needs
 * first == 1 and last == 1.  d_sums8_or_null: the layer's record on the DEVICE, 8-byte aligned, only read -- every workgroup computes the gains
 * from it itself, so no host wait stands between rsdsfm_seam_overlap_sums_dev and this call; NULL: no gain.  min_overlap >= 0 (0: 1024),
 * gain_mode 0 / 1, strength 1 .. 255 (0: 12).  d_cells_or_null: rows x cols cells, DEVICE, 8-byte aligned; NULL only with first && last.
 * first, last: 0 or 1.  At most 14 layers per `first` (see above).
 * d_image_out, d_mask_out, d_weight_or_null (rows x cols bytes), d_counts3_or_null are read only when last, and then every byte of the output
 * planes is written, so they need no preset.  d_counts3_or_null: a DEVICE array [unset, own only, averaged] of three int64, 8-byte aligned; the
 * call zeroes it (a memset on the context's stream) and the kernel adds to it -- a sum per workgroup with shuffles and LDS, then three 64-bit
 * integer atomics per workgroup: exact and independent of scheduling.
 * Every plane is 4-byte aligned; the outputs are distinct from the inputs, from the cells and from each other, the cells from the inputs.
 * One kernel launch (denoise_accumulate_kernel<CH, FIRST, LAST>), enqueued on the context's stream; returns without waiting.  A refused call
 * enqueues nothing.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased pointer, only one of the two layer pointers, no layer without first && last, channels, a
 * size outside [2, 16384], first or last other than 0 / 1, min_overlap < 0, gain_mode, strength outside its range. */
int rsdsfm_denoise_accumulate_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image_or_null,
                                  const uint8_t* d_layer_mask_or_null, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                                  int64_t min_overlap, int32_t gain_mode, int32_t strength, uint16_t* d_cells_or_null, int32_t first, int32_t last,
                                  uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, int64_t* d_counts3_or_null);

/* Kernel launches of rsdsfm_denoise_accumulate_dev: 1.  The memset of the counters is not counted.  Host only. */
int rsdsfm_denoise_accumulate_launches(void);

/* One denoised frame.  d_images, d_depths_colmajor, d_R_rows9, d_t_rows3: HOST arrays of nsrc DEVICE pointers, as rsdsfm_retime_frame_dev takes
 * them; the camera, rows, cols, mode, q5_mode and iterations are that call's.  nsrc 1 .. 15: source 0 is the own frame, the others its
 * neighbours.  M (nsrc x 9, row-major) and m (nsrc x 3): HOST, every source's pose in the target camera (rsdsfm_retime_poses' for the own frame,
 * rsdsfm_neighbour_poses' for the others).  window_or_null: (r0, c0, h, w), NULL = the full frame.
 * In order, on the context's stream:
 *   1. the reference image, mask and source plane (in the context's workspace) zeroed;
 *   2. the own frame rendered onto them with rsdsfm_stabilize_window_frame_dev (id 1, with the source plane); it never goes through the
 *      occlusion test;
 *   3. per neighbour: the layer zeroed; the neighbour rendered alone onto it with id 2 -- rsdsfm_stabilize_window_frame_dev with
 *      params->occlusion == 0, with 1 rsdsfm_stabilize_visible_frame_dev, or rsdsfm_stabilize_search_frame_dev when the context's
 *      rsdsfm_set_occlusion_search knob is 1, with params->occlusion_tol_q16 --; rsdsfm_seam_overlap_sums_dev into the layer's record;
 *      rsdsfm_denoise_accumulate_dev (first on the first neighbour, last on the last);
 *   4. with nsrc == 1 a single rsdsfm_denoise_accumulate_dev with no layer: the outputs are the window render's image and mask.
 * Every output is byte for byte those public calls made one after another.  The layer is the blended clip's layer (the retimer's layer A) of
 * the context's dense workspace; the reference planes (5 B per pixel) and the cells (8 B per pixel) join the workspace with the first call and
 * after a size change and are released by rsdsfm_destroy: a context that never asks keeps its footprint.  params->radius is not read here.
 * Returns without waiting.
 * RSDSFM_ERR_INVALID: nsrc outside [1, 15], a NULL array or entry, a misaligned source image, a source image that is an output, a NULL or
 * non-finite M / m, a window outside the frame, strength, gain_mode, occlusion, occlusion_tol_q16, min_overlap or radius outside its range, bad
 * struct_bytes, and the lists of the render calls and of rsdsfm_denoise_accumulate_dev. */
int rsdsfm_denoise_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                             const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                             int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_denoise_params* params_or_null,
                             const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, int64_t* d_counts3_or_null);

/* = nsrc rsdsfm_stabilize_window_launches(rows, cols) + 2 (nsrc - 1) (the sums and the accumulate per neighbour), or + 1 when nsrc == 1.
 * RSDSFM_ERR_INVALID for a size outside [2, 16384] or nsrc outside [1, 15].  Host only. */
int rsdsfm_denoise_launches(int32_t rows, int32_t cols, int32_t nsrc);

/* A clip, denoised AFTER it was solved: the call reads what rsdsfm_stabilize_video_dev or one of its variants left behind, as
 * rsdsfm_retime_video_dev does (d_frames, d_depth_maps, d_R, d_t: HOST arrays of nsources DEVICE pointers; the HOST arrays A, c, the path
 * A_path, c_path and scales; the camera, mode, q5_mode, iterations), and renders nsources frames: for q = 0 .. nsources - 1 in order the own
 * pose by rsdsfm_retime_poses(t = q), the neighbours and their poses by rsdsfm_neighbour_poses(q, params->radius) on the same path (the clip's
 * first and last frames have one-sided neighbours), then rsdsfm_denoise_frame_dev into d_out_images[q], d_out_masks[q] and
 * d_out_weights_or_null[q] (the array may be NULL).  The chain itself as the path (A_path = A, c_path = c) denoises the rectified frames in
 * place.  All poses are computed before anything is enqueued.  Every plane is byte for byte what the frame calls give when made one after
 * another.  counts_or_null: HOST, nsources x 3 int64 [unset, own only, averaged]; with it the call ends with one copy and one wait, without it
 * the call only enqueues.
 * RSDSFM_ERR_INVALID: a NULL array or entry, nsources < 1, what rsdsfm_retime_poses or rsdsfm_neighbour_poses refuses (a scale that is not
 * finite and positive, a non-finite pose), and the frame call's list. */
int rsdsfm_denoise_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                             double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                             const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                             const rsdsfm_denoise_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks,
                             uint8_t* const* d_out_weights_or_null, int64_t* counts_or_null);

#ifdef __cplusplus
}
#endif

/* the spatial top-up's declarations come with this header */
#include "rsdsfm_denoise_spatial.h"

#endif /* RSDSFM_DENOISE_H */
