/*
 * rsdsfm_erase.h -- C ABI of the mover removal on the MI355X: a frame of a solved clip WITHOUT what moved through it -- the clean plate's raw
 * flag (rsdsfm_plate.h) turned into a matte (speckle removed, grown, feathered), and the plate put under that matte while every other pixel
 * keeps the own frame's bytes.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  The
 * clean plate gives a median frame and a raw flag, and neither is what a user of a stabilised clip asks for: the plate is a median
 * everywhere -- static pixels lose their own bytes, the channels are selected independently, a region only the own frame saw is a one-candidate
 * median --, and the flag is raw -- a single hot pixel flags a 3 x 3 block, a mover's flag stops one pixel beyond its footprint, the edge is hard.
 *   matte       input a flag plane F (0 unset, 1 static, 2 moving, 3 undecided), open o 0 .. 3, grow g 0 .. 8, feather T 1 .. 16.
 *               seed      s(p) = F(p) == 2, or F(p) == 3 with include_undecided; every other byte value, values above 3 included, is no seed;
 *               core      core(p) = s(p') for every p' of the (2 o + 1)^2 window about p INSIDE the frame: pixels outside the frame do not veto,
 *                         so a mover at the border survives;
 *               distance  d(p) = the chessboard distance from p to the nearest core pixel, capped at C = o + g + T <= 27;
 *               matte     a(p) = clamp(C - d(p), 0, T): T within o + g of the core, one less per pixel beyond, 0 from distance C on.
 *               A 3 x 3 block of seeds (one hot pixel's flag) survives o = 0 and o = 1 and vanishes at o = 2.
 *   composite   the own frame in the target camera (image R, mask mR), the plate (image P, mask mP), the matte a, T, channels 1 or 3; a mask
 *               byte is set iff it is not 0, a matte byte above T counts as T.  Per pixel
 *                 mR unset                   image 0, mask 0                                            counted unset
 *                 mR set, a == 0             the bytes of R, mask 1                                     counted kept
 *                 mR set, a > 0, mP unset    the bytes of R, mask 1                                     counted unresolved
 *                 mR set, a > 0, mP set      out_c = (a P_c + (T - a) R_c + (T >> 1)) / T (floor), mask 1; a == T gives P_c exactly and is
 *                                            counted replaced, a < T is counted feathered
 *   counters    [unset, kept, replaced, feathered, unresolved]: five int64, exact.
 *   frame       rsdsfm_plate_frame_dev, the own frame through rsdsfm_stabilize_window_frame_dev, the matte of the plate's flag, the composite.
 * The defaults (open 2, grow 2, feather 4) are choices, not measurements.  Integers only on the device; tests/erase_spec_numpy.py is the
 * executable definition and every call here reproduces it bit for bit.  DESIGN.md section 12 ("Mover removal") has the kernels, the bytes, the
 * launches, the LDS and what the cross-compile shows.
 *
 * NOT here: temporal smoothing of the matte across frames; filling the own frame's empty band from the plate (where mR is unset the output is
 * unset); the matte fed into the denoise, the super-resolution or the fill; inpainting where every source saw the mover (the median of movers
 * is a mover); the C++ mirror.
 */
#ifndef RSDSFM_ERASE_H
#define RSDSFM_ERASE_H

#include "rsdsfm_plate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSDSFM_ERASE_OPEN_MAX 3
#define RSDSFM_ERASE_GROW_MAX 8
#define RSDSFM_ERASE_FEATHER_MAX 16
/* the defaults: choices, not measurements */
#define RSDSFM_ERASE_OPEN_DEFAULT 2
#define RSDSFM_ERASE_GROW_DEFAULT 2
#define RSDSFM_ERASE_FEATHER_DEFAULT 4

typedef struct rsdsfm_erase_params {
    int32_t radius;            /* the plate's: neighbours on each side for the clip call, 1 .. 7; 0: the default, 2 */
    int32_t threshold;         /* the plate's tau, 1 .. 255; 0: the default, 24 */
    int32_t min_votes;         /* the plate's, 1 .. 15; 0: the default, 3 */
    int32_t gain_mode;         /* the plate's: 0 every neighbour gain-matched to the own frame, the default; 1: off */
    int32_t occlusion;         /* the plate's: 0 the neighbours through rsdsfm_stabilize_window_frame_dev; 1: through the occlusion test */
    int32_t occlusion_tol_q16; /* the plate's: the occlusion test's tolerance, 1 .. 65536; 0: its default */
    int32_t struct_bytes;      /* 0 or sizeof(rsdsfm_erase_params), as rsdsfm_erase_params_init sets it; anything else is refused */
    int32_t open;              /* o, 1 .. 3; 0: the default, 2; -1: none (o = 0) */
    int64_t min_overlap;       /* the plate's, >= 0; 0: the default, 1024 */
    int32_t grow;              /* g, 1 .. 8; 0: the default, 2; -1: none (g = 0) */
    int32_t feather;           /* T, 1 .. 16; 0: the default, 4 */
    int32_t include_undecided; /* 0: only the flag 2 seeds the matte, the default; 1: the flag 3 too */
    int32_t reserved[5];       /* 0 */
} rsdsfm_erase_params;

/* The plate's defaults and open = 2, grow = 2, feather = 4, include_undecided = 0, struct_bytes = sizeof.  A NULL params pointer means these
 * values. */
int rsdsfm_erase_params_init(rsdsfm_erase_params* params);

/* The matte, as defined above.  d_flag: rows x cols bytes on the DEVICE, only read.  open 0 .. 3, grow 0 .. 8, feather 1 .. 16,
 * include_undecided 0 / 1: LITERAL values, no 0-means-default here.  d_matte_out: rows x cols bytes; every byte is written, no preset.
 * Both planes are 4-byte aligned and distinct.
 * THREE kernel launches on the context's stream -- matte_seed_cols_kernel (the seeds ANDed over the rows y - o .. y + o inside the frame),
 * matte_rows_kernel (the AND over the columns x - o .. x + o, then the distance along the row to the nearest core pixel), matte_cols_kernel
 * (the chessboard distance and the matte byte) -- through two rows x cols byte planes that join the context's dense workspace with the first
 * call: a context that never asks keeps its footprint.  Returns without waiting.  A refused call enqueues nothing.
 * RSDSFM_ERR_INVALID: a NULL, misaligned (4 B) or aliased plane, a size outside [2, 16384], open, grow, feather or include_undecided outside
 * its range. */
int rsdsfm_mover_matte_dev(rsdsfm_ctx* ctx, const uint8_t* d_flag, int32_t rows, int32_t cols, int32_t open, int32_t grow, int32_t feather,
                           int32_t include_undecided, uint8_t* d_matte_out);

/* Kernel launches of rsdsfm_mover_matte_dev: 3.  RSDSFM_ERR_INVALID for a size outside [2, 16384].  Host only. */
int rsdsfm_mover_matte_launches(int32_t rows, int32_t cols);

/* The composite, as defined above.  d_ref_image, d_plate_image: rows x cols x channels bytes, channels 1 or 3; d_ref_mask, d_plate_mask,
 * d_matte: rows x cols bytes; DEVICE, only read; image bytes under an unset mask byte never show.  feather 1 .. 16, literal: the T the matte
 * was made with.  d_image_out (rows x cols x channels), d_mask_out (rows x cols): every byte is written, no preset.  d_counts5_or_null: a
 * DEVICE array [unset, kept, replaced, feathered, unresolved] of five int64, 8-byte aligned; the call zeroes it (a memset on the context's
 * stream) and the kernel adds to it -- a sum per workgroup with shuffles and LDS, then at most five 64-bit integer atomics per workgroup: exact
 * and independent of scheduling.  Every plane is 4-byte aligned; every output is distinct from every input and from every other output; the
 * reference's and the plate's planes may not be the same plane twice (the reference's image as its mask), the plate may be the reference.
 * ONE kernel launch (erase_composite_kernel<CH>) on the context's stream; returns without waiting.  A refused call enqueues nothing.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased pointer (planes 4 B, counters 8 B), channels other than 1 / 3, a size outside
 * [2, 16384], feather outside [1, 16]. */
int rsdsfm_erase_composite_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_plate_image, const uint8_t* d_plate_mask,
                               const uint8_t* d_matte, int32_t channels, int32_t rows, int32_t cols, int32_t feather, uint8_t* d_image_out, uint8_t* d_mask_out,
                               int64_t* d_counts5_or_null);

/* Kernel launches of rsdsfm_erase_composite_dev: 1.  The memset of the counters is not counted.  Host only. */
int rsdsfm_erase_composite_launches(void);

/* One frame without its movers.  The sources, the camera, rows, cols, mode, q5_mode, iterations, nsrc, M, m and window_or_null exactly as
 * rsdsfm_plate_frame_dev takes them (source 0 is the own frame).  In order, on the context's stream:
 *   1. rsdsfm_plate_frame_dev with the plate's fields of the params into planes of the context's workspace: the plate's image, its mask and
 *      the flag -- the flag into d_moving_or_null when that is passed;
 *   2. the own frame in the target camera: rsdsfm_stabilize_window_frame_dev with id 1 on zeroed planes.  The plate call has just made
 *      exactly that render into its reference planes in the workspace, and they are read where they lie: no second render is enqueued;
 *   3. rsdsfm_mover_matte_dev of the flag into d_matte_or_null, or into a workspace plane without it;
 *   4. rsdsfm_erase_composite_dev into d_image_out, d_mask_out and d_counts5_or_null.
 * Every output is byte for byte those public calls made one after another.  The workspace planes (6 B per pixel beside the plate's) join the
 * workspace with the first call and are released by rsdsfm_destroy or a size change.  Every plane is 4-byte aligned, the counters 8; every
 * output is distinct from every source image and from every other output.  params->radius is not read here.  Returns without waiting; a
 * refused call enqueues nothing.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased output, open outside [-1, 3], grow outside [-1, 8], feather outside [0, 16],
 * include_undecided other than 0 / 1, bad struct_bytes, non-zero reserved words, and the list of rsdsfm_plate_frame_dev. */
int rsdsfm_erase_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                           const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                           int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_erase_params* params_or_null,
                           const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_matte_or_null, uint8_t* d_moving_or_null,
                           int64_t* d_counts5_or_null);

/* = rsdsfm_plate_launches(rows, cols, nsrc) + 3 (the matte) + 1 (the composite): step 2 enqueues nothing.
 * RSDSFM_ERR_INVALID for a size outside [2, 16384] or nsrc outside [1, 15].  Host only. */
int rsdsfm_erase_launches(int32_t rows, int32_t cols, int32_t nsrc);

/* A clip without its movers, AFTER it was solved: the clip exactly as rsdsfm_plate_video_dev takes and walks it -- for q = 0 .. nsources - 1 in
 * order the own pose by rsdsfm_retime_poses(t = q), the neighbours and their poses by rsdsfm_neighbour_poses(q, params->radius), then
 * rsdsfm_erase_frame_dev into d_out_images[q], d_out_masks[q], d_out_mattes_or_null[q] and d_out_moving_or_null[q] (either array may be NULL).
 * All poses are computed before anything is enqueued.  Every plane is byte for byte what the frame calls give when made one after another.
 * counts_or_null: HOST, nsources x 5 int64 [unset, kept, replaced, feathered, unresolved]; with it the call ends with one copy and one wait,
 * without it the call only enqueues.
 * RSDSFM_ERR_INVALID: a NULL array or entry, nsources < 1, an output plane that is a frame of the clip, what rsdsfm_retime_poses or
 * rsdsfm_neighbour_poses refuses, and the frame call's list. */
int rsdsfm_erase_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                           double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                           const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                           const rsdsfm_erase_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks,
                           uint8_t* const* d_out_mattes_or_null, uint8_t* const* d_out_moving_or_null, int64_t* counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_ERASE_H */
