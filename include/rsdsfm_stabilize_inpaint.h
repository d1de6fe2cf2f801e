/*
 * rsdsfm_stabilize_inpaint.h -- C ABI of the stabiliser's inpainting on the MI355X: the pixels of a stabilised frame that NO frame of the clip
 * saw, invented from what surrounds them.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  The
 * border fill (rsdsfm_stabilize_fill.h), the crop (rsdsfm_stabilize_crop.h) and the blend (rsdsfm_stabilize_blend.h) take pixels from the
 * frames of the clip; what none of them shows stays black with a mask byte of 0.  Here an integer pull-push pyramid -- the dense rectifier's
 * stage A (rsdsfm_rectify_dense.h), for bytes instead of inverse depths -- gives every such pixel a value.  The call is generic: any image of
 * 1 or 3 channels and any validity mask, the output of rsdsfm_rectify_dense_frame_dev included.
 *   level 0     v = byte << 8 per channel; a cell is valid iff its mask byte is not 0 (one validity for all channels)
 *   pull        level l (h x w) -> level l + 1 (ceil(h / 2) x ceil(w / 2)), down to 1 x 1: a cell has up to four children (those outside
 *               the level are absent); with n valid children v = (sum of the valid children + (n >> 1)) / n per channel and the cell is
 *               valid; with n = 0 it is invalid
 *   push        from coarse to fine; the 1 x 1 level is complete if it is valid.  An invalid cell (y, x) of level l takes from the complete
 *               level l + 1 (hc x wc), with yn = y >> 1, yf = clamp(yn + (y odd ? 1 : -1), 0, hc - 1) and xn, xf alike,
 *               v = (9 c[yn, xn] + 3 c[yn, xf] + 3 c[yf, xn] + c[yf, xf] + 8) >> 4: the dense rectifier's sample position
 *               ((x + 1/2) / 2 - 1/2, replicate border) with exact weights.  A valid cell keeps its value.
 *   output      an empty pixel of level 0 gets (v + 128) >> 8 per channel and, in the source plane when one is passed, the byte
 *               RSDSFM_SOURCE_INPAINTED; a set pixel keeps its bytes; the mask is only read -- it stays the record of what was seen;
 *               count = the pixels written
 *   nothing set the 1 x 1 level is invalid: nothing is written, count = 0
 * Every level value is at most 65280: 16 bits per channel, no clamp anywhere.  Integers only: tests/stabilize_inpaint_spec_numpy.py is the
 * executable definition and every call here reproduces it bit for bit.  DESIGN.md section 12 ("Inpaint") has the kernels, the launches, the
 * bytes and what has been measured.
 *
 * NOT here: exemplar, patch or diffusion inpainting (the values are a smooth interpolation: no texture is invented), temporal consistency of
 * the invented pixels (every frame is inpainted alone), the C++ mirror.  The clip's last frame is built since: rsdsfm_last_frame.h.
 */
#ifndef RSDSFM_STABILIZE_INPAINT_H
#define RSDSFM_STABILIZE_INPAINT_H

#include "rsdsfm_stabilize_blend.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the source byte of an inpainted pixel.  The clip calls use ids <= 33 (radius 16): nothing clashes */
#define RSDSFM_SOURCE_INPAINTED 255

/* The empty pixels (d_mask byte 0; rows x cols bytes, DEVICE, only read) of d_image_inout (rows x cols x channels bytes, channels 1 or 3,
 * DEVICE) filled as defined above; rows and cols in [2, 16384].  d_source_or_null: rows x cols bytes on the DEVICE, RSDSFM_SOURCE_INPAINTED
 * written where a pixel was; d_count_or_null: one int64 on the DEVICE, 8-byte aligned, overwritten with the number of pixels written.
 * Every plane is 4-byte aligned and the planes are distinct.  Enqueues rsdsfm_inpaint_launches(rows, cols) kernels on the context's stream
 * and returns without waiting; the first of them zeroes the counter, the last adds to it, and the last reads the 1 x 1 level's validity on
 * the device, so a frame without a set pixel needs no host wait.  The pyramid (8 bytes per cell, about 2.7 bytes per pixel) lives in the
 * context's dense workspace: made when first asked for, made again when the size changes, released by rsdsfm_destroy.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased pointer, channels other than 1 or 3, a size outside its range. */
int rsdsfm_inpaint_frame_dev(rsdsfm_ctx* ctx, uint8_t* d_image_inout, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols,
                             uint8_t* d_source_or_null, int64_t* d_count_or_null);

/* Kernel launches of rsdsfm_inpaint_frame_dev: level 0 -> 1, the large pulls, the single-workgroup launch, the large pushes, the output
 * (3 for a small frame, 8 at 1280 x 720).  Memsets are not counted.  RSDSFM_ERR_INVALID for a size outside [2, 16384].  Host only. */
int rsdsfm_inpaint_launches(int32_t rows, int32_t cols);

/* A whole clip, cropped, zoomed, blended and inpainted: rsdsfm_stabilize_video_blended_dev (its arguments up to blend_counts_or_null, its
 * results, its rules, its errors) made unchanged, then for p = 0 .. nframes - 2 in order:
 *   - d_blend_images[p] copied to d_inpaint_images[p] (rows x cols x channels bytes) and, when d_inpaint_sources_or_null is passed,
 *     d_blend_sources[p] to d_inpaint_sources_or_null[p] (rows x cols bytes), device to device;
 *   - rsdsfm_inpaint_frame_dev on the copy with d_blend_masks[p].
 * Every output is byte for byte what those public calls give when made one after another; everything the inner call writes is what it writes
 * alone.  No window (h = 0): the blend planes are zero, so the inpaint planes are zero and the counts 0.
 * inpaint_counts_or_null: HOST, nframes - 1 int64, the pixels written per frame; with it the call ends with one copy and one wait, without
 * it the passes are only enqueued.
 * RSDSFM_ERR_INVALID in addition: a NULL or misaligned inpaint plane, an inpaint plane that is one of the frame's blend planes or its other
 * inpaint plane.
 * With stabilize_params_or_null->last_frame == 1 the inner call renders the last frame too (rsdsfm_stabilize.h), the crop search takes nframes
 * masks, rsdsfm_neighbour_poses is asked with nframes "pairs" and every per-frame loop runs p = 0 .. nframes - 1.  d_inpaint_images, d_inpaint_sources_or_null and inpaint_counts_or_null
 * then have nframes entries (rows), like the inner call's per-frame arrays; results, d_flows, seeds, the check masks, records and broken keep
 * nframes - 1 (nframes - 2 for the links).  The rule "byte for byte those public calls one after another" holds as it stands. */
int rsdsfm_stabilize_video_inpainted_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                         double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                         const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows, double* const* d_depth_maps,
                                         double* const* d_R, double* const* d_t, rsdsfm_frame_result* results,
                                         const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks_or_null,
                                         const rsdsfm_link_params* link_params_or_null, rsdsfm_link_record* records, double* scales, double* A, double* c,
                                         uint8_t* broken_or_null, const rsdsfm_fuse_params* fuse_params_or_null, double* const* d_fused_maps_or_null,
                                         const rsdsfm_stabilize_params* stabilize_params_or_null, int mode, int q5_mode, int32_t iterations, double* A_s,
                                         double* c_s, double* M, double* m, uint8_t* const* d_stab_images, uint8_t* const* d_masks_out,
                                         int64_t* valid_or_null, const rsdsfm_stabilize_fill_params* fill_params_or_null, uint8_t* const* d_sources_or_null,
                                         int64_t* counts_or_null, const rsdsfm_stabilize_crop_params* crop_params_or_null, const int32_t* window_in_or_null,
                                         uint8_t* const* d_crop_images, uint8_t* const* d_crop_masks, uint8_t* const* d_crop_sources_or_null,
                                         int32_t window_out[4], int64_t* crop_counts_or_null, const rsdsfm_stabilize_blend_params* blend_params_or_null,
                                         uint8_t* const* d_blend_images, uint8_t* const* d_blend_masks, uint8_t* const* d_blend_sources, uint32_t* gains_or_null,
                                         int64_t* blend_counts_or_null, uint8_t* const* d_inpaint_images, uint8_t* const* d_inpaint_sources_or_null,
                                         int64_t* inpaint_counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_STABILIZE_INPAINT_H */
