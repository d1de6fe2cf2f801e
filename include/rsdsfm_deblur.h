/*
 * rsdsfm_deblur.h -- C ABI of the sharpness transfer on the MI355X: a frame of a solved clip that the camera's shake blurred takes pixels from
 * its neighbours in time where a neighbour is sharper, every neighbour rendered ALONE into the frame's own (virtual) camera through its depth
 * map and rolling-shutter pose table (Matsushita, Ofek, Ge, Tang, Shum, "Full-frame video stabilization with motion inpainting", 2006,
 * section 5: measure how blurred each frame is relative to its neighbours, transfer from the sharper ones).
 *
 * The reference solves one pair per process run (evaluateSingleRun's per-pair loop, main.cc:380-523) and has no counterpart to this.  Every
 * stage behind the stabiliser treats an input frame as sharp; the shake the stabiliser removes also blurs single frames, and on the smoothed
 * path those frames show as "blur pumping".  The temporal denoise cannot stand in: its patch weight is the mean ABSOLUTE difference, which
 * reads the detail a blurred frame lacks as disagreement and leaves the blurred bytes as they are.
 *   inputs      per step the denoise's (rsdsfm_denoise.h): the reference (R, mR), one layer (L, mL), the layer's 8-word overlap record, the
 *               gains G_c and gained bytes k_c = min(255, (G_c L_c + 32768) >> 16) with the same gain_mode and min_overlap;
 *               v(p) = mR(p) set and mL(p) set; Y_R(p) = sum_c R_c(p), Y_L(p) = sum_c k_c(p).
 *   sharpness   T = [pairs, A_R, A_L, 0], four uint64: over every pixel p with v(p) and each of its two forward neighbours
 *               q in {p + (0, 1), p + (1, 0)} inside the frame with v(q): pairs += 1, A_R += (Y_R(p) - Y_R(q))^2, A_L += (Y_L(p) - Y_L(q))^2.
 *               Every adjacent pair both images see counts once, on the same support for both.  Squared, so that edges outweigh sensor noise.
 *   tau         the layer's factor: 0 when pairs < min_pairs or 16 A_L <= (16 + margin) A_R, else min(32, (16 (A_L - A_R)) / max(A_R, 1)):
 *               16 at twice the own frame's sharpness, 32 at three times or more, 0 for a layer that equals the reference.
 *   gate        D(p) = |sum (Y_R - Y_L)(p')| and N(p) = channels #{p'} over the p' of the 3 x 3 window about p inside the frame with v(p');
 *               w(p) = 16 - min(16, (16 D) / (h N)) where v(p), else 0: the denoise's form with a SIGNED patch sum, a low-pass comparison
 *               that passes detail the own frame has lost and still rejects a mover or a gross misregistration.  h: the strength.
 *               gate_mode 1: w = 16 wherever v (the classical method).
 *   cell        rsdsfm_shutter.h's layout, the denoise's steps with u = (w tau + 8) >> 4 in the place of w:
 *               first [16 R_c, 16] where mR is set, else 0; every step s_c += u k_c, n += u; last out_c = (2 s_c + n) / (2 n) and mask 1
 *               where n > 0, else 0 / 0; the weight plane is n; the counters [unset: n == 0, own only: n == 16, transferred: n > 16].
 *               With at most RSDSFM_DEBLUR_LAYERS_MAX = 7 layers per `first` n <= 16 + 7 * 32 = 240 and s_c <= 61 200, the denoise's bounds.
 *               THE CALLER OF rsdsfm_deblur_accumulate_dev KEEPS TO 7 LAYERS per `first`; the call cannot count them.
 * Consequences: when every layer has tau = 0 the output is the own frame's bytes and mask exactly; no order of the layers changes a byte;
 * with tau = 16, u = w; a sharp frame among blurred neighbours keeps its bytes.  Integers only on the device; tests/deblur_spec_numpy.py is
 * the executable definition and every call here reproduces it bit for bit.  DESIGN.md section 12 ("Sharpness transfer") has the kernels.
 *
 * The defaults (margin 4, strength 24, the cap 32, radius 2) are choices, not measurements.
 *
 * Per scanline band (built since; tests/deblur_bands_spec_numpy.py is the definition, DESIGN.md section 12 "Sharpness per scanline band"): the
 * rows of a rolling-shutter frame are exposed one after another, so shake blurs a frame differently down its rows, and one tau per layer is
 * either 0 for the whole frame or a diluted value everywhere.  With band_rows = H, a multiple of 16 in [16, 16384]:
 *   bands        band(y) = y / H, NB = ceil(rows / H) <= RSDSFM_DEBLUR_BANDS_MAX = 64; the last band may be short.
 *   band records NB x 4 uint64, T_b = [pairs, A_R, A_L, 0]: the pairs of the sharpness record above, every pair (p, q) in the band of p, its
 *                left or upper pixel (a vertical pair across a band border belongs to the upper band).  The sum of the T_b is T, exactly.
 *   band tau     tau_b = tau(T_b) with the same margin and the same min_pairs, applied to the band.  No new knob.
 *   row tau      centres c_b = b H + H / 2 (also for a short last band); tau(y) = tau_0 for y < c_0, tau_{NB-1} for y >= c_{NB-1}, else with
 *                b = (y - H / 2) / H and f = (y - H / 2) - b H: tau(y) = (tau_b (H - f) + tau_{b+1} f + H / 2) / H, an integer in 0 .. 32.  The
 *                interpolation keeps a band border from showing as a horizontal seam in sharpness.
 *   step         the step above with u(p) = (w(p) tau(row of p) + 8) >> 4; u <= 32 per layer as before, so n <= 240, s_c <= 61 200 and the
 *                limit of 7 layers per `first` hold unchanged.
 * Consequences: NB = 1 gives the unbanded accumulate's bytes; every tau_b = 0 gives the own frame's bytes; no order of the layers changes a
 * byte; a row both of whose surrounding bands have tau = 0 keeps its bytes.
 *
 * The band height's default (0: off) and the linear interpolation between band centres are choices, not measurements, too.
 *
 * NOT here: deconvolution or any single-frame sharpening; gates wider than 3 x 3 (a blur much wider than the window reads partly as
 * disagreement); the mover flag fed into the gate; the C++ mirror.
 */
#ifndef RSDSFM_DEBLUR_H
#define RSDSFM_DEBLUR_H

#include "rsdsfm_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSDSFM_DEBLUR_RADIUS_MAX 3
#define RSDSFM_DEBLUR_LAYERS_MAX 7
#define RSDSFM_DEBLUR_TAU_MAX 32
#define RSDSFM_DEBLUR_MARGIN_MAX 64
#define RSDSFM_DEBLUR_BANDS_MAX 64
/* the defaults: choices, not measurements */
#define RSDSFM_DEBLUR_RADIUS_DEFAULT 2
#define RSDSFM_DEBLUR_STRENGTH_DEFAULT 24
#define RSDSFM_DEBLUR_MARGIN_DEFAULT 4
#define RSDSFM_DEBLUR_MIN_PAIRS_DEFAULT 1024

typedef struct rsdsfm_deblur_params {
    int32_t radius;            /* neighbours on each side for the clip call, 1 .. 3; 0: the default, 2 */
    int32_t strength;          /* the gate's h, 1 .. 255; 0: the default, 24 */
    int32_t margin;            /* sixteenths by which a neighbour must be sharper, 1 .. 64; -1: none (0); 0: the default, 4 (a quarter) */
    int32_t gate_mode;         /* 0: the gate, the default; 1: off, w = 16 wherever both masks are set */
    int32_t gain_mode;         /* 0: every neighbour gain-matched to the own frame on their overlap, the default; 1: off */
    int32_t occlusion;         /* 0: the neighbours through rsdsfm_stabilize_window_frame_dev; 1: through the occlusion test */
    int32_t occlusion_tol_q16; /* the occlusion test's tolerance, 1 .. 65536; 0: its default */
    int32_t struct_bytes;      /* 0 or sizeof(rsdsfm_deblur_params), as rsdsfm_deblur_params_init sets it; anything else is refused */
    int64_t min_overlap;       /* overlap pixels below which a neighbour gets no gain, >= 0; 0: the default, 1024 (the blend's) */
    int64_t min_pairs;         /* pixel pairs below which a neighbour's tau is 0, >= 0; 0: the default, 1024 */
    int32_t band_rows;         /* rows per scanline band, a multiple of 16 in [16, 16384] with at most 64 bands; 0: off, one tau per neighbour */
    int32_t reserved[3];       /* 0 */
} rsdsfm_deblur_params;

/* radius = 2, strength = 24, margin = 4, gate_mode = 0, gain_mode = 0, occlusion = 0, occlusion_tol_q16 = 0, min_overlap = 1024,
 * min_pairs = 1024, band_rows = 0, struct_bytes = sizeof.  A NULL params pointer means these values. */
int rsdsfm_deblur_params_init(rsdsfm_deblur_params* params);

/* The sharpness record of one layer against the reference, as defined above.  d_ref_image, d_layer_image: rows x cols x channels bytes,
 * channels 1 or 3; d_ref_mask, d_layer_mask: rows x cols bytes; DEVICE, 4-byte aligned, only read.  d_sums8_or_null: the layer's overlap
 * record on the DEVICE (rsdsfm_seam_overlap_sums_dev), 8-byte aligned, only read -- every workgroup computes the gains from it itself, so no host
 * wait stands in front of this call; NULL: no gain.  min_overlap >= 0 (0: 1024), gain_mode 0 / 1.  d_sharp4_out: four uint64 on the DEVICE,
 * 8-byte aligned, distinct from every input.  One memset (the record) and one launch (deblur_sharpness_kernel<CH>: a sum per workgroup with
 * shuffles and LDS, then three 64-bit integer atomics per workgroup: exact and independent of scheduling), enqueued on the context's stream;
 * returns without waiting.  A refused call enqueues nothing.
 * RSDSFM_ERR_INVALID: a NULL, misaligned or aliased pointer, channels other than 1 / 3, a size outside [2, 16384], min_overlap < 0, gain_mode. */
int rsdsfm_deblur_sharpness_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image, const uint8_t* d_layer_mask,
                                int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null, int64_t min_overlap, int32_t gain_mode,
                                uint64_t* d_sharp4_out);

/* tau of a record, as defined above.  Host only, no context, like rsdsfm_seam_gains.  sharp4: HOST.  margin: the params' word (-1: none,
 * 0: the default, 1 .. 64); min_pairs >= 0 (0: the default).  RSDSFM_ERR_INVALID: a NULL pointer, margin or min_pairs outside its range. */
int rsdsfm_deblur_tau(const uint64_t* sharp4, int32_t margin, int64_t min_pairs, int32_t* tau_out);

/* One step, as defined above: rsdsfm_denoise_accumulate_dev's arguments, its rules and its refusals, with strength 1 .. 255 (0: 24), and
 * d_sharp4_or_null: the layer's sharpness record on the DEVICE, 8-byte aligned, only read, REQUIRED when a layer is given -- one thread of
 * every workgroup computes tau from it (one 64-bit integer division), so no host wait stands between rsdsfm_deblur_sharpness_dev and this
 * call; margin and min_pairs as rsdsfm_deblur_tau takes them; gate_mode 0 / 1.  A launch with tau = 0 that is neither first nor last returns
 * after reading the record: a blurred neighbour costs no image bytes.  At most 7 layers per `first`.
 * One kernel launch (deblur_accumulate_kernel<CH, FIRST, LAST>), enqueued on the context's stream; returns without waiting.  A refused call
 * enqueues nothing.
 * RSDSFM_ERR_INVALID: the list of rsdsfm_denoise_accumulate_dev, a layer without its sharpness record, a misaligned or aliased record,
 * margin, min_pairs or gate_mode outside its range. */
int rsdsfm_deblur_accumulate_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image_or_null,
                                 const uint8_t* d_layer_mask_or_null, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                                 int64_t min_overlap, int32_t gain_mode, int32_t strength, const uint64_t* d_sharp4_or_null, int32_t margin, int64_t min_pairs,
                                 int32_t gate_mode, uint16_t* d_cells_or_null, int32_t first, int32_t last, uint8_t* d_image_out, uint8_t* d_mask_out,
                                 uint8_t* d_weight_or_null, int64_t* d_counts3_or_null);

/* One frame: rsdsfm_denoise_frame_dev's arguments and rules with nsrc 1 .. 8.  In order, on the context's stream: the reference planes zeroed
 * and the own frame rendered onto them (id 1, with the source plane; never through the occlusion test); per neighbour the layer zeroed, the
 * neighbour rendered alone onto it (the window render, the occlusion test or the search, as the denoise chooses),
 * rsdsfm_seam_overlap_sums_dev, rsdsfm_deblur_sharpness_dev, rsdsfm_deblur_accumulate_dev (first on the first neighbour, last on the last);
 * with nsrc == 1 a single rsdsfm_deblur_accumulate_dev with no layer.  Every output is byte for byte those public calls made one after
 * another.  d_sharp_records_or_null: DEVICE, (nsrc - 1) x 4 uint64, 8-byte aligned; neighbour j's record lands at entry j, else in a record of
 * the workspace.  The reference planes, the cells and the layer are the denoise's planes of the context's dense workspace, the workspace's
 * sharpness record (32 B) joins it with the first call: a context that never asks keeps its footprint.  params->radius is not read here.
 * Returns without waiting.
 * With params->band_rows > 0 the two band calls stand where rsdsfm_deblur_sharpness_dev and rsdsfm_deblur_accumulate_dev stand (the launches are
 * the same, rsdsfm_deblur_launches is unchanged), d_sharp_records_or_null is (nsrc - 1) x NB x 4 uint64 with neighbour j's band records at entry
 * j NB, and without it the band records live in a 2 KB plane of the workspace (64 x 32 B), made with the first such call.
 * RSDSFM_ERR_INVALID: nsrc outside [1, 8], a params field outside its range, bad struct_bytes, a band_rows that is neither 0 nor a multiple of
 * 16 in [16, 16384] or gives more than 64 bands, a misaligned record array or one that is an output, and the list of rsdsfm_denoise_frame_dev. */
int rsdsfm_deblur_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                            const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                            int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_deblur_params* params_or_null,
                            const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, int64_t* d_counts3_or_null,
                            uint64_t* d_sharp_records_or_null);

/* The band records of one layer against the reference, as defined above ("per scanline band"): rsdsfm_deblur_sharpness_dev's arguments, checks
 * and refusals, with band_rows and d_band_records_out: NB x 4 uint64 on the DEVICE, NB = ceil(rows / band_rows), 8-byte aligned, distinct from every
 * input.  One memset (NB x 32 B) and one launch (deblur_band_sharpness_kernel<CH>: the sharpness kernel with the workgroup's three sums added to
 * record (16 blockIdx.y) / band_rows; the same three 64-bit integer atomics per workgroup: exact and independent of scheduling), enqueued on the
 * context's stream; returns without waiting.  A refused call enqueues nothing.
 * RSDSFM_ERR_INVALID: the list of rsdsfm_deblur_sharpness_dev, a band_rows that is no multiple of 16 in [16, 16384], more than 64 bands. */
int rsdsfm_deblur_band_sharpness_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image, const uint8_t* d_layer_mask,
                                     int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null, int64_t min_overlap, int32_t gain_mode,
                                     int32_t band_rows, uint64_t* d_band_records_out);

/* tau of each of nbands band records (records: HOST, nbands x 4; taus_out: HOST, nbands): rsdsfm_deblur_tau per record.  Host only, no context.
 * RSDSFM_ERR_INVALID: a NULL pointer, nbands outside [1, 64], margin or min_pairs outside its range. */
int rsdsfm_deblur_band_taus(const uint64_t* records, int32_t nbands, int32_t margin, int64_t min_pairs, int32_t* taus_out);

/* tau of each of `rows` rows from the band taus, the interpolation defined above (taus: HOST, nbands, each 0 .. 32; row_taus_out: HOST, rows).
 * Host only, no context.  RSDSFM_ERR_INVALID: a NULL pointer, a band_rows that is no multiple of 16 in [16, 16384], rows outside [2, 16384],
 * nbands other than ceil(rows / band_rows) or above 64, a tau outside [0, 32]. */
int rsdsfm_deblur_row_taus(const int32_t* taus, int32_t nbands, int32_t band_rows, int32_t rows, int32_t* row_taus_out);

/* One step with a tau per row: rsdsfm_deblur_accumulate_dev's arguments, rules, checks and refusals (the same limit of 7 layers per `first`),
 * with d_band_records_or_null, the layer's NB x 4 band records on the DEVICE (rsdsfm_deblur_band_sharpness_dev), in the record's place, and
 * band_rows.  Three threads of every workgroup compute the taus of the tile's band and of the bands above and below it (one 64-bit integer
 * division each), sixteen the tile's row taus; no read leaves the NB records.  A launch that is neither first nor last returns after reading the
 * records where all three taus are 0: a blurred band of a sharp neighbour costs no image bytes.  With NB = 1 every byte, the cells included, is
 * rsdsfm_deblur_accumulate_dev's.  One kernel launch (deblur_band_accumulate_kernel<CH, FIRST, LAST>), enqueued on the context's stream; returns
 * without waiting.  A refused call enqueues nothing.
 * RSDSFM_ERR_INVALID: the list of rsdsfm_deblur_accumulate_dev, a band_rows that is no multiple of 16 in [16, 16384], more than 64 bands. */
int rsdsfm_deblur_band_accumulate_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image_or_null,
                                      const uint8_t* d_layer_mask_or_null, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                                      int64_t min_overlap, int32_t gain_mode, int32_t strength, const uint64_t* d_band_records_or_null, int32_t band_rows,
                                      int32_t margin, int64_t min_pairs, int32_t gate_mode, uint16_t* d_cells_or_null, int32_t first, int32_t last,
                                      uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, int64_t* d_counts3_or_null);

/* = nsrc rsdsfm_stabilize_window_launches(rows, cols) + 3 (nsrc - 1) (the sums, the sharpness and the accumulate per neighbour), or + 1 when
 * nsrc == 1.  RSDSFM_ERR_INVALID for a size outside [2, 16384] or nsrc outside [1, 8].  Host only. */
int rsdsfm_deblur_launches(int32_t rows, int32_t cols, int32_t nsrc);

/* A solved clip: rsdsfm_denoise_video_dev's arguments and its walk (for q = 0 .. nsources - 1 the own pose by rsdsfm_retime_poses(t = q), the
 * neighbours and their poses by rsdsfm_neighbour_poses(q, params->radius), then rsdsfm_deblur_frame_dev) into d_out_images[q],
 * d_out_masks[q] and d_out_weights_or_null[q].  Every plane is byte for byte what the frame calls give when made one after another.
 * counts_or_null: HOST, nsources x 3 int64 [unset, own only, transferred].  taus_or_null: HOST, nsources x 6 int32: entry j of frame q is
 * the tau of the j-th neighbour rsdsfm_neighbour_poses lists for q (nearer first, previous before next; a neighbour outside the clip is not
 * listed), -1 behind the listed ones.  The taus are computed on the host by rsdsfm_deblur_tau from the records, which are copied with the
 * counts: with either array the call ends with one copy and one wait, without both it only enqueues.
 * RSDSFM_ERR_INVALID: the lists of rsdsfm_denoise_video_dev and rsdsfm_deblur_frame_dev. */
int rsdsfm_deblur_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                            double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                            const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                            const rsdsfm_deblur_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks,
                            uint8_t* const* d_out_weights_or_null, int64_t* counts_or_null, int32_t* taus_or_null);

/* rsdsfm_deblur_video_dev with the band taus: band_taus_or_null: HOST, nsources x 6 x NB int32, NB = ceil(rows / params->band_rows): band b of the
 * j-th listed neighbour of frame q at [(q 6 + j) NB + b], -1 behind the listed neighbours.  taus_or_null then gets the MAX over the bands of
 * each listed neighbour's taus.  The per-frame device words are 3 + 4 * 6 * NB; with any of the three arrays the call ends with one copy and
 * one wait.  rsdsfm_deblur_video_dev with band_rows > 0 is this call with NULL.  With band_rows = 0 both are the unbanded call and
 * band_taus_or_null is filled as if NB = 1 (nsources x 6).
 * RSDSFM_ERR_INVALID: the list of rsdsfm_deblur_video_dev. */
int rsdsfm_deblur_video_banded_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx,
                                   double fy, double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t,
                                   const double* A, const double* c, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode,
                                   int32_t iterations, const rsdsfm_deblur_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images,
                                   uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null, int64_t* counts_or_null, int32_t* taus_or_null,
                                   int32_t* band_taus_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_DEBLUR_H */
