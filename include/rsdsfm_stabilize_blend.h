/*
 * rsdsfm_stabilize_blend.h -- C ABI of the stabiliser's seam blend on the MI355X: the photometry at the seam between a stabilised frame and
 * what the border fill takes from its neighbours.
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  The
 * border fill (rsdsfm_stabilize_fill.h) and the crop (rsdsfm_stabilize_crop.h) copy a neighbour's pixels next to the own frame's with a hard
 * edge; the edge moves from frame to frame, and real clips change exposure between frames, so the band flickers.  Here every candidate is
 * rendered ALONE onto a layer (rsdsfm_stabilize_window_frame_dev, unchanged), gets one gain per channel from the pixels it shares with the
 * own frame, and is mixed into the own frame over the `feather` pixels next to the own frame's empty band:
 *   dist(y, x)  0 where the own frame's mask is 0, else min(T, chessboard distance max(|dy|, |dx|) to the nearest empty pixel OF THE FRAME);
 *               the frame's own edge is not a hole (the crop's margin has the same convention).  T = feather.
 *   sums        [count, sum image_c (c < channels), sum layer_c (c < channels), 0 ...], 8 uint64, over the pixels whose source byte is 1 (the
 *               own frame's, not yet blended) and whose layer mask is not 0
 *   G_c         clamp((sum image_c 65536 + (sum layer_c >> 1)) / sum layer_c, 16384, 262144), in 1 / 65536; 65536 when gain_mode is 1, when
 *               count < min_overlap or when sum layer_c is 0
 *   per pixel with a set layer mask, k_c = min(255, (G_c layer_c + 32768) >> 16):
 *               source 0                  image = k, mask = 1, source = source_id                                        (filled)
 *               source 1 and dist < T     image_c = (dist image_c + (T - dist) k_c + (T >> 1)) / T, source = source_id   (blended)
 *               otherwise                 nothing: deep inside the own frame, or a nearer candidate already has the pixel
 * A pixel is blended at most once, and the image still holds the own frame's bytes there when it is.  With feather 1 nothing is ever blended;
 * with the gain off as well a layer call is the fill's hard copy.  Integers only: tests/stabilize_blend_spec_numpy.py is the executable
 * definition and every call here reproduces it bit for bit.  DESIGN.md section 12 ("Seam blend") has the kernels, the launches, the bytes
 * and what has been measured.
 *
 * NOT here: feathering between two neighbours' regions, multi-band blending, gains smoothed over time or solved jointly over the clip,
 * vignetting, occlusion tests between candidates (built since: rsdsfm_stabilize_visible.h), the clip's last frame (built since: rsdsfm_last_frame.h), inpainting of pixels nobody saw (built since:
 * rsdsfm_stabilize_inpaint.h).
 */
#ifndef RSDSFM_STABILIZE_BLEND_H
#define RSDSFM_STABILIZE_BLEND_H

#include "rsdsfm_stabilize_crop.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsdsfm_stabilize_blend_params {
    int64_t min_overlap;  /* overlap pixels below which a candidate gets no gain, >= 0; 0: the default, 1024 (a choice, not a measurement) */
    int32_t feather;      /* T, 1 .. 64; 0: the default, 16 (a choice, not a measurement) */
    int32_t gain_mode;    /* 0: compensate, the default; 1: off */
    int32_t struct_bytes; /* 0 (zero-initialised struct: every default) or sizeof(rsdsfm_stabilize_blend_params), as
                             rsdsfm_stabilize_blend_params_init sets it; anything else is refused */
    int32_t reserved[3];  /* 0 */
} rsdsfm_stabilize_blend_params;

/* min_overlap = 1024, feather = 16, gain_mode = 0, struct_bytes = sizeof */
int rsdsfm_stabilize_blend_params_init(rsdsfm_stabilize_blend_params* params);

/* The distance plane of one DEVICE mask of rows x cols bytes (0 = empty, anything else set), rows and cols in [2, 16384], feather 1 .. 64 (0:
 * the default, 16), into d_dist_out (rows x cols bytes, DEVICE); both 4-byte aligned and distinct.  Enqueues two kernels on
 * the context's stream -- the distance along every row, into a plane of the context's dense workspace (made when first asked for and released
 * by rsdsfm_destroy), then the minimum down the columns -- and returns without waiting.  The mask is only read.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased pointer, a size or feather outside its range. */
int rsdsfm_seam_distance_dev(rsdsfm_ctx* ctx, const uint8_t* d_mask, int32_t rows, int32_t cols, int32_t feather, uint8_t* d_dist_out);

/* Kernel launches of rsdsfm_seam_distance_dev: 2.  RSDSFM_ERR_INVALID for a size outside [2, 16384].  Host only. */
int rsdsfm_seam_distance_launches(int32_t rows, int32_t cols);

/* One candidate's layer (d_layer_image: rows x cols x channels bytes, channels 1 or 3; d_layer_mask: rows x cols bytes; both only read) onto
 * the in-out planes as defined above, with d_dist a plane of rsdsfm_seam_distance_dev for the SAME feather as params_or_null's (NULL: the
 * defaults).  source_id is 2 .. 255.  d_source_inout and d_sums_out are REQUIRED; d_sums_out is 8 uint64 on the DEVICE, 8-byte aligned, and
 * receives the sums.  d_counts_or_null: 2 int64 on the DEVICE, 8-byte aligned, overwritten with [filled, blended].  Every plane is 4-byte
 * aligned; the layer planes and d_dist may not be one of the in-out planes, which are distinct.  Enqueues one memset (the sums), the sums
 * kernel (which also zeroes the counters) and the blend kernel, which computes the gains from the sums itself, on the context's stream and
 * returns without waiting.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased pointer, channels, a size, source_id, feather, gain_mode or min_overlap outside its range,
 * bad struct_bytes. */
int rsdsfm_seam_blend_layer_dev(rsdsfm_ctx* ctx, const uint8_t* d_layer_image, const uint8_t* d_layer_mask, int32_t channels, int32_t rows, int32_t cols,
                                const uint8_t* d_dist, const rsdsfm_stabilize_blend_params* params_or_null, int32_t source_id, uint8_t* d_image_inout,
                                uint8_t* d_mask_inout, uint8_t* d_source_inout, uint64_t* d_sums_out, int64_t* d_counts_or_null);

/* Kernel launches of rsdsfm_seam_blend_layer_dev: 2.  The memset is not counted.  RSDSFM_ERR_INVALID for a size outside [2, 16384].  Host
 * only. */
int rsdsfm_seam_blend_layer_launches(int32_t rows, int32_t cols);

/* HOST only: the gains of one record (sums8: 8 values as rsdsfm_seam_blend_layer_dev writes them, copied back by the caller) with the kernel's
 * own integer arithmetic; channels 1 or 3, min_overlap and gain_mode as in the params (0: 1024; 0 or 1).  gains_out[c] for c >= channels is
 * 65536.  RSDSFM_ERR_INVALID: a NULL pointer, channels, min_overlap < 0, gain_mode. */
int rsdsfm_seam_gains(const uint64_t* sums8, int32_t channels, int64_t min_overlap, int32_t gain_mode, uint32_t gains_out[3]);

/* A whole clip, cropped, zoomed and blended: rsdsfm_stabilize_video_cropped_dev (its arguments up to crop_counts_or_null, its results, its
 * rules, its errors) made unchanged, then for p = 0 .. nframes - 2 in order, through window_out:
 *   - d_blend_images[p] (rows x cols x channels bytes), d_blend_masks[p] and d_blend_sources[p] (REQUIRED) zeroed;
 *   - the own frame's rsdsfm_stabilize_window_frame_dev (rsdsfm_virtual_poses' pose, id 1, with the source plane) into them;
 *   - rsdsfm_seam_distance_dev of d_blend_masks[p] into a plane of the context's workspace;
 *   - per neighbour of rsdsfm_neighbour_poses, in its order: the context's layer image and mask zeroed, the neighbour's
 *     rsdsfm_stabilize_window_frame_dev onto the layer with its id and no source plane, and rsdsfm_seam_blend_layer_dev --
 * on the FUSED maps when d_fused_maps_or_null is passed.  Every output is byte for byte what those public calls give when made one after
 * another; everything the inner call writes is what it writes alone.  No window (h = 0): the blend planes are zeroed; to blend without
 * cropping pass the full-frame window (0, 0, rows, cols) as window_in_or_null.  With a fill radius of 0 the blend output is the own render.
 * gains_or_null: HOST, (nframes - 1) x 2 radius x 3 uint32, per frame and offset -1, +1, -2, +2, ... the gains the layer got (computed as
 * rsdsfm_seam_gains does from the records copied back); 65536 for a skipped offset or an unused channel.
 * blend_counts_or_null: HOST, (nframes - 1) x (2 + 4 radius) int64, per frame [none, own_untouched, (filled, blended) per offset -1, +1, -2,
 * +2, ...]; none and own_untouched are computed on the host from the own render's count.
 * With neither host array the passes are only enqueued; with either the call ends with one copy and one wait.
 * RSDSFM_ERR_INVALID in addition: a NULL or misaligned blend plane, a source plane that is the mask, bad blend params.
 * With stabilize_params_or_null->last_frame == 1 the inner call renders the last frame too (rsdsfm_stabilize.h), the crop search takes nframes
 * masks, rsdsfm_neighbour_poses is asked with nframes "pairs" and every per-frame loop runs p = 0 .. nframes - 1.  d_blend_images, d_blend_masks, d_blend_sources, gains_or_null and blend_counts_or_null
 * then have nframes entries (rows), like the inner call's per-frame arrays; results, d_flows, seeds, the check masks, records and broken keep
 * nframes - 1 (nframes - 2 for the links).  The rule "byte for byte those public calls one after another" holds as it stands. */
int rsdsfm_stabilize_video_blended_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
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
                                       int64_t* blend_counts_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_STABILIZE_BLEND_H */
