/*
 * rsdsfm_plate_medoid.h -- C ABI of the clean plate's COLOUR-CONSISTENT estimator on the MI355X: where rsdsfm_plate_median_dev (rsdsfm_plate.h)
 * selects every channel of a plate pixel on its own, so that a BGR pixel may mix channels of different sources -- candidates grey (100, 100, 100),
 * red (0, 0, 255) and blue (255, 0, 0) give (100, 0, 100), a purple no frame ever showed --, this one selects a WHOLE candidate: the L1 medoid,
 * the candidate whose summed L1 distance to the other candidates is smallest.  The reference has no counterpart (see rsdsfm_plate.h).
 *   gains, candidates, n, mask, votes   exactly rsdsfm_plate.h's: k_jc = min(255, (G_jc L_jc + 32768) >> 16), the own pixel takes part where mR != 0.
 *   plate       where n >= 1: for every valid candidate i, cost_i = sum over the valid j of sum_c |v_ic - v_jc| (at most 14 * 3 * 255 = 10710),
 *               colour_i = v_i0 | v_i1 << 8 | v_i2 << 16 (the pixel's little-endian packed dword), and P(p) is the colour of the candidate with the
 *               smallest key_i = (cost_i << 24) | colour_i.  Two candidates with equal keys have equal colours: P depends on the multiset of
 *               candidate colours only, neither the order of the layers nor any tie changes a byte.  Where n == 0 image 0 and mask 0.
 *   moving, counters   rsdsfm_plate.h's v, e, D, N, the flags 0 / 3 / 2 / 1 and [unset, static, moving, undecided], word for word, with this P.
 *   consequences   with one channel the medoid is the lower median (the sum of absolute deviations is smallest at every median; for an even n both
 *               middle values tie on cost and the smaller key is the smaller value): channels == 1 runs plate_median_kernel, the same bytes.
 *               With two candidates the plate is the one with the smaller packed colour, not the per-channel minimum.
 * Integers only on the device, no division; tests/plate_medoid_spec_numpy.py is the executable definition and every call here reproduces it bit
 * for bit.  DESIGN.md section 12 ("Colour-consistent plate") has the kernel, the registers, the bytes and the launches.
 *
 * NOT here: weighted medoids; a geometric median that is not a candidate; a plane that says which source was chosen (ambiguous under ties); the
 * estimator as a field of rsdsfm_plate_params or rsdsfm_erase_params (their reserved words stay 0) -- it is a knob of the context.
 */
#ifndef RSDSFM_PLATE_MEDOID_H
#define RSDSFM_PLATE_MEDOID_H

#include "rsdsfm_plate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSDSFM_PLATE_MEDIAN 0 /* the per-channel lower median, the default */
#define RSDSFM_PLATE_MEDOID 1 /* the L1 medoid */

/* The medoid, as defined above.  Every argument is rsdsfm_plate_median_dev's and means what it means there; so do the checks, the refusals
 * and the contract: every byte of every plane given is written (no preset), d_counts4_or_null is zeroed by a memset on the context's stream
 * and added to by the kernel, without d_moving_or_null and d_counts4_or_null the flag is not computed.
 * ONE kernel launch (channels == 3: plate_medoid_kernel<3, LAYERS, FLAG>; channels == 1: plate_median_kernel<1, LAYERS, FLAG>), enqueued on
 * the context's stream; returns without waiting.  A refused call enqueues nothing.
 * RSDSFM_ERR_INVALID: rsdsfm_plate_median_dev's list. */
int rsdsfm_plate_medoid_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* const* d_layer_images,
                            const uint8_t* const* d_layer_masks, int32_t nlayers, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                            int64_t min_overlap, int32_t gain_mode, int32_t threshold, int32_t min_votes, uint8_t* d_image_out, uint8_t* d_mask_out,
                            uint8_t* d_votes_or_null, uint8_t* d_moving_or_null, int64_t* d_counts4_or_null);

/* Kernel launches of rsdsfm_plate_medoid_dev: 1.  The memset of the counters is not counted.  Host only. */
int rsdsfm_plate_medoid_launches(void);

/* Which estimator rsdsfm_plate_frame_dev ends with: RSDSFM_PLATE_MEDIAN (0, the default: every byte of every call is what it is without this
 * call) or RSDSFM_PLATE_MEDOID (1: step 4 of rsdsfm_plate_frame_dev is one rsdsfm_plate_medoid_dev in place of the rsdsfm_plate_median_dev).
 * rsdsfm_plate_video_dev, rsdsfm_erase_frame_dev and rsdsfm_erase_video_dev follow it through rsdsfm_plate_frame_dev: their outputs stay byte
 * for byte the public calls made one after another, with rsdsfm_plate_medoid_dev in the median's place.  rsdsfm_plate_median_dev itself never
 * changes, and neither does a launch count.  Holds until set again.
 * RSDSFM_ERR_INVALID: any other value; the knob stays where it was. */
int rsdsfm_set_plate_estimator(rsdsfm_ctx* ctx, int32_t estimator);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_PLATE_MEDOID_H */
