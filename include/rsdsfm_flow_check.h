/*
 * rsdsfm_flow_check.h -- C ABI of the forward-backward flow check on the MI355X: which vectors of a DeepFlow field can be trusted, and a
 * field in which the others are (0, 0), so that the solve leaves them out (its flatten keeps a pixel only if |flow|^2 > flow_threshold) and
 * they carry no depth.
 *
 * A variational flow fills occlusions, disocclusions, pixels whose motion leaves the frame and independently moving objects with smooth
 * but wrong vectors.  The check (Sundaram, Brox, Keutzer, ECCV 2010) follows the forward vector of pixel (i, j) to its landing point in
 * frame 2, takes the bilinear sample (bu, bv) of the BACKWARD field (frame 2 -> frame 1) there and keeps the pixel iff the landing point
 * lies in the frame and
 *      |f + b|^2 <= a1 * (|f|^2 + |b|^2) + a2           (a1 = 0.01, a2 = 0.5 by default).
 * tests/flow_check_spec_numpy.py is the executable definition, operation by operation, in float64; the kernel
 * (csrc/flow_check_kernels.hip) reproduces it bit for bit.  NaN and infinities reject their pixel.  DESIGN.md section 12 ("Forward-backward
 * flow check") has the bytes per pixel, the launches, the workspace and what has been measured.  There is no motion-boundary criterion, and the
 * dense rectifier does not read the mask.
 *
 * Alignment: masks are written as packed 32-bit words: 4-byte aligned (RSDSFM_ERR_INVALID otherwise).
 */
#ifndef RSDSFM_FLOW_CHECK_H
#define RSDSFM_FLOW_CHECK_H

#include "rsdsfm_video.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsdsfm_flow_check_params {
    double a1; /* share of |f|^2 + |b|^2 the residual may reach; finite, >= 0 */
    double a2; /* constant part of the bound, squared pixels; finite, >= 0 */
} rsdsfm_flow_check_params;

/* a1 = 0.01, a2 = 0.5 */
int rsdsfm_flow_check_default_params(rsdsfm_flow_check_params* out);

/* The check alone, on device fields: d_fwd (frame 1 -> 2) and d_bwd (frame 2 -> 1), rows x cols x 2 doubles each, (u, v) per pixel,
 * row-major -- rsdsfm_deep_flow_dev's layout.  Outputs: d_mask rows x cols bytes (1 = consistent); optional d_masked_flow_or_null
 * rows x cols x 2 doubles (the forward vector where the mask is 1, else (0, 0)), d_resid_or_null rows x cols doubles (|f + b|^2 where
 * the landing point is inside and the value finite, else +inf), d_count_or_null one int64 (the number of ones: zeroed on the stream in
 * front of the launch, added to with integer atomics, so exact).  One launch, enqueued on the context's stream; returns without waiting.
 * d_masked_flow_or_null may equal d_fwd (in place); every other output that equals an input or another output is RSDSFM_ERR_INVALID, as
 * are rows or cols outside [2, 16384], a NULL required pointer, a misaligned mask, a parameter that is negative or not finite. */
int rsdsfm_flow_consistency_dev(rsdsfm_ctx* ctx, const double* d_fwd, const double* d_bwd, int32_t rows, int32_t cols,
                                const rsdsfm_flow_check_params* params_or_null, uint8_t* d_mask, double* d_masked_flow_or_null, double* d_resid_or_null,
                                int64_t* d_count_or_null);

/* rsdsfm_deep_flow_dev both ways, then the check: d_flow receives the MASKED forward field (rsdsfm_solve_frame_dev can follow on the same
 * stream and buffer), d_mask and d_count_or_null as above, d_bwd_or_null the backward field (NULL = a context-owned buffer of 16 bytes per
 * pixel, allocated on first use and when the size changes, released by rsdsfm_destroy).  The two fields are bit for bit
 * rsdsfm_deep_flow_dev(d_img1, d_img2) and rsdsfm_deep_flow_dev(d_img2, d_img1): they are that call's launches, twice, on its workspace.
 * Arguments and errors as rsdsfm_deep_flow_dev's and the check's; d_flow, d_bwd_or_null, d_mask and d_count_or_null must differ. */
int rsdsfm_deep_flow_checked_dev(rsdsfm_ctx* ctx, const uint8_t* d_img1, const uint8_t* d_img2, int32_t rows, int32_t cols, int32_t channels,
                                 const rsdsfm_flow_params* flow_params_or_null, const rsdsfm_flow_check_params* check_params_or_null, double* d_flow,
                                 double* d_bwd_or_null, uint8_t* d_mask, int64_t* d_count_or_null);

/* rsdsfm_solve_video_dev (its arguments up to `results`, its rules, its errors) with the check between the flow and the solve of every
 * batch: the forward fields of the batch, the backward fields (the same frames through the reversed pointer array: every launch serves
 * the whole batch), ONE check launch for all pairs of the batch, then the solve of the batch on the masked fields.  d_masks: nframes - 1
 * device pointers, rows x cols bytes each, 4-byte aligned (required).  d_flows_or_null[p] (or the library's ring) holds the MASKED field
 * of pair p.  d_bwd_flows_or_null: where the backward fields go (nframes - 1 device buffers), NULL = a library-owned ring of B buffers.
 * consistent_or_null: nframes - 1 host int64, the count of every pair, filled before the call returns.
 * results[p], d_depth_maps[p] and the pose tables are bit for bit what rsdsfm_solve_frame_dev gives on rsdsfm_deep_flow_checked_dev's
 * output for that pair and seed, at every batch size and lane count. */
int rsdsfm_solve_video_checked_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                   double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                   const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows_or_null,
                                   double* const* d_depth_maps, double* const* d_R_or_null, double* const* d_t_or_null, rsdsfm_frame_result* results,
                                   const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks, double* const* d_bwd_flows_or_null,
                                   int64_t* consistent_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_FLOW_CHECK_H */
