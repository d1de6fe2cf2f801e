/*
 * rsdsfm_plate.h -- C ABI of the clean plate on the MI355X: a frame of a solved clip with what moved taken out -- the per-pixel, per-channel
 * MEDIAN of the own frame and its neighbours in time, every neighbour rendered ALONE into the frame's own (virtual) camera through its depth map
 * and rolling-shutter pose table -- and a per-pixel "this moved" flag.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  Every
 * other multi-frame stage here (fill, blend, retime, shutter, denoise, super-resolution) is a weighted mean of registered frames: a person walking
 * through a hand-held clip stays in every output frame and nothing tells a caller where they are.  A median over the registered candidates gives
 * both the frame without them and the place where they were.
 *   inputs      the reference (image R, mask mR: the own frame in the target camera) and L layers, 0 <= L <= RSDSFM_PLATE_LAYERS_MAX = 14 (image
 *               L_j, mask mL_j: a neighbour rendered alone); a mask byte is set iff it is not 0, image bytes under an unset mask byte never show.
 *               One 8-word record per layer, [count, sum image_c, sum layer_c, 0 ...], as rsdsfm_seam_overlap_sums_dev writes it.
 *   gains       per layer and channel G_jc from the layer's record as rsdsfm_seam_gains computes it (clamped to [16384, 262144]; 65536 with
 *               gain_mode == 1, count < min_overlap, sum layer_c == 0, or no record): the denoise's gain exactly;
 *               k_jc(p) = min(255, (G_jc L_jc(p) + 32768) >> 16).
 *   candidates  at pixel p: R_c(p) if mR(p) is set, and k_jc(p) for every j with mL_j(p) set; n(p) their number, 0 .. 15.
 *   plate       where n >= 1: per channel P_c(p) = the LOWER MEDIAN of the candidate values of that channel, the element at index (n - 1) >> 1
 *               of their ascending order, and mask 1; where n == 0 image 0 and mask 0.  The votes plane is n.  Per channel, so the plate depends
 *               on the multiset of values only: neither the order of the layers nor any tie changes a byte.  The plate is also set where the
 *               own frame is empty and a neighbour saw the pixel.
 *   moving      v(p) = mR(p) set and n(p) >= min_votes; e(p) = sum_c |R_c(p) - P_c(p)| where v(p); D(p) = sum of e(p') and N(p) = channels #{p'}
 *               over the p' of the 3 x 3 window about p inside the frame with v(p') -- the denoise's D and N.  One byte per pixel:
 *               0 where mR(p) is unset; 3 (undecided) where mR(p) is set and N(p) == 0; 2 (moving) where D(p) > threshold N(p); 1 (static)
 *               otherwise.  A comparison of integer products, no division.  threshold 1 .. 255 (0: the default, 24, the retimer's conflict
 *               threshold); min_votes 1 .. 15 (0: the default, 3: below three candidates a median outvotes nobody).  Choices, not measurements.
 *   counters    [unset, static, moving, undecided]: the pixels with flag 0, 1, 2, 3; four int64.
 *   frame       the own frame through rsdsfm_stabilize_window_frame_dev, every neighbour alone on its own zeroed layer of a stack, a record per
 *               layer by rsdsfm_seam_overlap_sums_dev, one median over all of them.
 * Integers only on the device; tests/plate_spec_numpy.py is the executable definition and every call here reproduces it bit for bit.  DESIGN.md
 * section 12 ("Clean plate") has the kernel, the bytes, the launches, the LDS layout and what the ISA shows for the selection.
 *
 * NOT here: the flag fed back into the denoise, the super-resolution or the fill; a vector (colour-consistent) median -- the channels are
 * selected independently -- (built since: rsdsfm_plate_medoid.h, the L1 medoid, and rsdsfm_set_plate_estimator, which puts it in step 4 of
 * rsdsfm_plate_frame_dev); weighted medians; temporal smoothing or morphology of the flag; inpainting where every source saw the mover (the
 * median of movers is a mover); the C++ mirror.
 */
#ifndef RSDSFM_PLATE_H
#define RSDSFM_PLATE_H

#include "rsdsfm_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSDSFM_PLATE_RADIUS_MAX 7
#define RSDSFM_PLATE_LAYERS_MAX 14
/* the defaults: choices, not measurements */
#define RSDSFM_PLATE_RADIUS_DEFAULT 2
#define RSDSFM_PLATE_THRESHOLD_DEFAULT 24
#define RSDSFM_PLATE_MIN_VOTES_DEFAULT 3

typedef struct rsdsfm_plate_params {
    int32_t radius;            /* neighbours on each side for the clip call, 1 .. 7; 0: the default, 2 */
    int32_t threshold;         /* tau, 1 .. 255; 0: the default, 24 */
    int32_t min_votes;         /* candidates a pixel needs to take part in the flag, 1 .. 15; 0: the default, 3 */
    int32_t gain_mode;         /* 0: every neighbour gain-matched to the own frame on their overlap, the default; 1: off */
    int32_t occlusion;         /* 0: the neighbours through rsdsfm_stabilize_window_frame_dev; 1: through the occlusion test */
    int32_t occlusion_tol_q16; /* the occlusion test's tolerance, 1 .. 65536; 0: its default */
    int32_t struct_bytes;      /* 0 or sizeof(rsdsfm_plate_params), as rsdsfm_plate_params_init sets it; anything else is refused */
    int32_t reserved0;         /* 0 */
    int64_t min_overlap;       /* overlap pixels below which a neighbour gets no gain, >= 0; 0: the default, 1024 (the blend's) */
    int32_t reserved[4];       /* 0 */
} rsdsfm_plate_params;

/* radius = 2, threshold = 24, min_votes = 3, gain_mode = 0, occlusion = 0, occlusion_tol_q16 = 0, min_overlap = 1024, struct_bytes = sizeof.
 * A NULL params pointer means these values. */
int rsdsfm_plate_params_init(rsdsfm_plate_params* params);

/* The median, as defined above.  d_ref_image: rows x cols x channels bytes, channels 1 or 3; d_ref_mask: rows x cols bytes; DEVICE, only read.
 * d_layer_images, d_layer_masks: HOST arrays of nlayers DEVICE pointers (planes of the reference's sizes, only read); both may be NULL only
 * with nlayers == 0, and then the plate is the reference.  d_sums8_or_null: nlayers x 8 uint64 on the DEVICE, 8-byte aligned, only read, record
 * j for layer j -- every workgroup computes the gains from the records itself, so no host wait stands between rsdsfm_seam_overlap_sums_dev and
 * this call; NULL: no gain.  min_overlap >= 0 (0: 1024), gain_mode 0 / 1, threshold 0 .. 255 (0: 24), min_votes 0 .. 15 (0: 3).
 * d_image_out (rows x cols x channels), d_mask_out, d_votes_or_null, d_moving_or_null (rows x cols bytes): every byte of every plane given is
 * written, so they need no preset.  d_counts4_or_null: a DEVICE array [unset, static, moving, undecided] of four int64, 8-byte aligned; the call
 * zeroes it (a memset on the context's stream) and the kernel adds to it -- a sum per workgroup with shuffles and LDS, then four 64-bit integer
 * atomics per workgroup: exact and independent of scheduling.  Without d_moving_or_null and d_counts4_or_null the flag is not computed.
 * Every plane is 4-byte aligned; every output is distinct from every input, from the records and from every other output.
 * ONE kernel launch (plate_median_kernel<CH, LAYERS, FLAG>), enqueued on the context's stream; returns without waiting.  A refused call
 * enqueues nothing.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased pointer (planes 4 B, records and counters 8 B), a NULL layer array or entry with
 * nlayers > 0, nlayers outside [0, 14], channels other than 1 / 3, a size outside [2, 16384], min_overlap < 0, gain_mode, threshold or
 * min_votes outside its range. */
int rsdsfm_plate_median_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* const* d_layer_images,
                            const uint8_t* const* d_layer_masks, int32_t nlayers, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                            int64_t min_overlap, int32_t gain_mode, int32_t threshold, int32_t min_votes, uint8_t* d_image_out, uint8_t* d_mask_out,
                            uint8_t* d_votes_or_null, uint8_t* d_moving_or_null, int64_t* d_counts4_or_null);

/* Kernel launches of rsdsfm_plate_median_dev: 1.  The memset of the counters is not counted.  Host only. */
int rsdsfm_plate_median_launches(void);

/* One clean plate.  d_images, d_depths_colmajor, d_R_rows9, d_t_rows3: HOST arrays of nsrc DEVICE pointers, as rsdsfm_denoise_frame_dev takes
 * them; the camera, rows, cols, mode, q5_mode and iterations are that call's.  nsrc 1 .. 15: source 0 is the own frame, the others its
 * neighbours.  M (nsrc x 9, row-major) and m (nsrc x 3): HOST, every source's pose in the target camera.  window_or_null: (r0, c0, h, w), NULL =
 * the full frame.
 * In order, on the context's stream:
 *   1. the reference image, mask and source plane (in the context's workspace) zeroed, and the own frame rendered onto them with
 *      rsdsfm_stabilize_window_frame_dev (id 1, with the source plane); it never goes through the occlusion test;
 *   2. per neighbour j: ITS OWN layer of the stack zeroed; the neighbour rendered alone onto it with id 2 --
 *      rsdsfm_stabilize_window_frame_dev with params->occlusion == 0, with 1 rsdsfm_stabilize_visible_frame_dev, or
 *      rsdsfm_stabilize_search_frame_dev when the context's rsdsfm_set_occlusion_search knob is 1, with params->occlusion_tol_q16, exactly as
 *      the denoise chooses between them --;
 *   3. rsdsfm_seam_overlap_sums_dev into record j;
 *   4. one rsdsfm_plate_median_dev over the nsrc - 1 layers.
 * Every output is byte for byte those public calls made one after another.  The reference planes (5 B per pixel), the stack of
 * (channels + 1) rows cols bytes per layer and the records join the workspace with the first call, grow when a call brings more neighbours than
 * any before it, are made again after a size change, and are released by rsdsfm_destroy: a context that never asks keeps its footprint.
 * params->radius is not read here.  Returns without waiting.
 * RSDSFM_ERR_INVALID: nsrc outside [1, 15], a NULL array or entry, a misaligned source image, a source image that is an output, a NULL or
 * non-finite M / m, a window outside the frame, threshold, min_votes, gain_mode, occlusion, occlusion_tol_q16, min_overlap or radius outside its
 * range, bad struct_bytes, and the lists of the render calls and of rsdsfm_plate_median_dev. */
int rsdsfm_plate_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                           const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                           int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_plate_params* params_or_null,
                           const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_votes_or_null, uint8_t* d_moving_or_null,
                           int64_t* d_counts4_or_null);

/* = nsrc rsdsfm_stabilize_window_launches(rows, cols) + (nsrc - 1) (the sums per neighbour) + 1 (the median).
 * RSDSFM_ERR_INVALID for a size outside [2, 16384] or nsrc outside [1, 15].  Host only. */
int rsdsfm_plate_launches(int32_t rows, int32_t cols, int32_t nsrc);

/* A clip's plates, AFTER it was solved: the call reads what rsdsfm_stabilize_video_dev or one of its variants left behind, as
 * rsdsfm_denoise_video_dev does (d_frames, d_depth_maps, d_R, d_t: HOST arrays of nsources DEVICE pointers; the HOST arrays A, c, the path
 * A_path, c_path and scales; the camera, mode, q5_mode, iterations), and renders nsources plates: for q = 0 .. nsources - 1 in order the own
 * pose by rsdsfm_retime_poses(t = q), the neighbours and their poses by rsdsfm_neighbour_poses(q, params->radius) on the same path (the clip's
 * first and last frames have one-sided neighbours), then rsdsfm_plate_frame_dev into d_out_images[q], d_out_masks[q], d_out_votes_or_null[q] and
 * d_out_moving_or_null[q] (either array may be NULL).  All poses are computed before anything is enqueued.  Every plane is byte for byte what
 * the frame calls give when made one after another.  counts_or_null: HOST, nsources x 4 int64 [unset, static, moving, undecided]; with it the
 * call ends with one copy and one wait, without it the call only enqueues.
 * RSDSFM_ERR_INVALID: a NULL array or entry, nsources < 1, an output plane that is a frame of the clip, what rsdsfm_retime_poses or
 * rsdsfm_neighbour_poses refuses (a scale that is not finite and positive, a non-finite pose), and the frame call's list. */
int rsdsfm_plate_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                           double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                           const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                           const rsdsfm_plate_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks,
                           uint8_t* const* d_out_votes_or_null, uint8_t* const* d_out_moving_or_null, int64_t* counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_PLATE_H */
