/*
 * rsdsfm_fuse.h -- C ABI of the fusion of a clip's depth maps on the MI355X: every pair's map with its holes filled from what the
 * neighbouring pairs measured there, and per-pixel flags that say who measured a pixel and whether the neighbours agree.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  A
 * pair's depth map (rsdsfm_solve_video_dev's) carries a depth only where the pair's RANSAC kept the pixel.  The link
 * (rsdsfm_trajectory.h) already moves pair p's depth to its second capture and looks it up in pair p + 1's map to form a ratio; the
 * fusion keeps that measurement.  For pair p:
 *   PREV  pair p - 1's depths, moved to that pair's second capture by its solved motion (the link's steps 1 - 4), times the link's ratio,
 *         splatted at the pixels its flow lands on; the smallest offer per pixel wins (the nearest surface)
 *   NEXT  pair p + 1's depth where pair p's own flow lands, divided by the link's ratio and moved back (the link's step 3 solved for z)
 *   fused = the own depth where there is one (bit for bit), else PREV, else NEXT, else +0.0
 * OWN > PREV > NEXT because a hole's own vector is the one the RANSAC rejected, so a value gathered along it is poor, while a splatted
 * value travels along the previous pair's inlier vectors ("Depth fusion", has the measured errors).  All pairs are
 * fused from the ORIGINAL maps: no value travels more than one pair.  tests/fuse_spec_numpy.py is the executable definition, operation by
 * operation, in float64; the kernels (csrc/fuse_kernels.hip) reproduce every output bit for bit.
 *
 * There is no clip entry point of its own: the clip form is rsdsfm_solve_video_linked_dev followed by rsdsfm_fuse_depths_dev on its
 * fields, maps, motions and records.  rsdsfm_rectify_dense_frame_dev and rsdsfm_link_pairs_dev take a fused map like any other.
 */
#ifndef RSDSFM_FUSE_H
#define RSDSFM_FUSE_H

#include "rsdsfm_trajectory.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the bits of a pixel's flag byte */
#define RSDSFM_FUSE_OWN 1          /* the pair's own map has a valid depth (finite, > 0) */
#define RSDSFM_FUSE_PREV 2         /* a candidate from the previous pair exists */
#define RSDSFM_FUSE_NEXT 4         /* a candidate from the next pair exists */
#define RSDSFM_FUSE_PREV_AGREES 8  /* ... and agrees with the fused value f: a <= f (1 + tol) and a (1 + tol) >= f */
#define RSDSFM_FUSE_NEXT_AGREES 16 /* (a candidate that is itself the fused value agrees) */

typedef struct rsdsfm_fuse_params {
    double tol;           /* agreement of a candidate with the fused value; finite, >= 0 (0.1, the link's) */
    int32_t struct_bytes; /* 0 (zero-initialised struct) or sizeof(rsdsfm_fuse_params), as rsdsfm_fuse_params_init sets it; anything else is
                             refused: the caller was built against another layout */
    int32_t reserved;     /* 0 */
} rsdsfm_fuse_params;

/* tol = 0.1, struct_bytes = sizeof */
int rsdsfm_fuse_params_init(rsdsfm_fuse_params* params);

typedef struct rsdsfm_fuse_record {
    int64_t own;          /* pixels with a depth of the pair's own */
    int64_t filled_prev;  /* holes filled from the previous pair */
    int64_t filled_next;  /* holes filled from the next pair (the previous one offered nothing) */
    int64_t confirmed;    /* own pixels with at least one candidate that agrees */
    int64_t contradicted; /* own pixels with a candidate that does not agree (a pixel can be both) */
    int64_t left;         /* pixels without a value */
} rsdsfm_fuse_record;

/* The fused maps of npairs >= 1 solved pairs.  Arguments as rsdsfm_link_pairs_dev's: d_fields[p] rows x cols x 2 doubles, row-major
 * (d_fields[npairs - 1] is not read and may be NULL); d_depth_maps[p] rows x cols doubles, column-major; v_3n / w_3n / k_n the pairs' final
 * motions (HOST); global_shutter: whether the solve ran with use_global_shutter_mode.  records: the npairs - 1 link records (HOST;
 * rsdsfm_link_pairs_dev's); a link is USED iff valid is set and ratio is finite and > 0 (rsdsfm_chain_clip's rule), and no value crosses
 * any other.  With one pair records may be NULL and the fused map is the own map.
 * Outputs, each written in full:  d_fused_maps[p]: rows x cols doubles, column-major (+0.0 = no value); none of them may be an input map
 * (pair p reads Z_{p+1} as the solve left it).  d_flags_or_null[p]: rows x cols bytes, row-major.  d_splat_planes_or_null[l], l < npairs - 1:
 * rows x cols uint64, row-major: the bit pattern of the winning offer of pair l to pair l + 1, all ones where nothing landed (and
 * everywhere for a link that is not used); NULL = planes of the context's workspace (8 bytes per pixel, at most 32 in flight; made on
 * first use, released by rsdsfm_destroy).  out_records_or_null: npairs HOST records.
 * Pairs run in chunks of 32: a preset of the chunk's planes, ONE splat launch and ONE merge launch per chunk, no host wait in between.
 * With out_records_or_null the counters come back in one copy behind the last launch, which the call waits for; without it the call only
 * enqueues on the context's stream.  Exact and independent of scheduling: integer atomics only.
 * RSDSFM_ERR_INVALID: npairs < 1, a side outside [2, 16384], a NULL required pointer, an output that is an input or another output, tol
 * negative or not finite, bad struct_bytes. */
int rsdsfm_fuse_depths_dev(rsdsfm_ctx* ctx, const double* const* d_fields, const double* const* d_depth_maps, const double* v_3n, const double* w_3n,
                           const double* k_n, int32_t npairs, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double gamma,
                           int32_t global_shutter, const rsdsfm_link_record* records, const rsdsfm_fuse_params* params_or_null,
                           double* const* d_fused_maps, uint8_t* const* d_flags_or_null, uint64_t* const* d_splat_planes_or_null,
                           rsdsfm_fuse_record* out_records_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_FUSE_H */
