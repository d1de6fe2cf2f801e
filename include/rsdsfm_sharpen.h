/*
 * rsdsfm_sharpen.h -- C ABI of the sharpen stage on the MI355X: a noise-gated unsharp mask whose coring threshold follows the noise curve
 * (rsdsfm_noise_curve.h, which this header includes).
 *
 * Every image stage behind the solve leaves its frame softer than its source: the stabiliser, the fill, the crop and the retimer sample
 * bilinearly, the super-resolution never undoes the sensor's blur, both denoisers average.  The sharpness transfer helps only where a neighbour
 * is sharper.  This stage restores local contrast in ONE frame; it cores its detail signal below a threshold proportional to the strength
 * h(level of the pixel), so the noise the curve measured is not amplified, and it limits the result to the local 3 x 3 range, so edges do not
 * overshoot.  The reference has no counterpart.  tests/sharpen_spec_numpy.py is the executable definition; every call here reproduces it bit
 * for bit.  Integers only.
 *   inputs      image I (rows x cols x channels bytes, channels 1 or 3), mask m, v(p) = m(p) != 0; amount_q4 0 .. 64 (16 = 1.0), coring_q4
 *               0 .. 64, overshoot 0 .. 255; the strength h: one number 1 .. 255, or one per pixel from a curve.
 *   blur        k = [1, 4, 6, 4, 1], k(o) = k[oy + 2] k[ox + 2] for o in [-2, 2]^2.  Over the o with p + o inside the frame and v(p + o):
 *               S_c(p) = sum k(o) I_c(p + o), K(p) = sum k(o).
 *   detail      d_c = K I_c(p) - S_c: scaled by K, nothing is divided yet.
 *   threshold   the level of p is its byte (gray) or (b + g + r + 1) / 3 (BGR), as the noise curve's consumers take it; h the fixed strength or
 *               entry `level` of the 256-entry table of rsdsfm_noise_curve_strengths, formed on the device as the curve top-up forms it;
 *               T = (coring_q4 h + 8) >> 4, the same for every channel.
 *   coring      soft: e_c = max(0, |d_c| - T K).
 *   gain        r_c = (2 amount_q4 e_c + 16 K) / (32 K) in integer division: the magnitude rounded half up; o_c = I_c(p) + sign(d_c) r_c.
 *   limit       lo_c, hi_c: the minimum and maximum of I_c over the set pixels of the 3 x 3 block about p inside the frame, p included;
 *               out_c = clamp(o_c, max(0, lo_c - overshoot), min(255, hi_c + overshoot)).
 *   outputs     out where v(p); 0 in every channel where not.  The mask is the input's and is not written.
 *   counters    [unset, kept, sharpened, limited], exclusive, summing to rows cols.  unset: not v(p); kept: out == I in every channel;
 *               limited: not kept and the limit changed o_c in some channel; sharpened: the rest.
 *   bounds      K <= 256 (the kernel's sum); where v(p), K >= 36 (the centre tap) and K >= 121 on a full mask (a corner keeps 11 x 11 of
 *               16 x 16).  d_c = sum over o != 0 of k(o) (I_c(p) - I_c(p + o)), so |d_c| <= 255 (K - 36) <= 56 100 < 65 280.
 *               T <= (64 * 255 + 8) >> 4 = 1020, but e_c = 0 as soon as T >= 255, and the kernel clamps T to 255: T K <= 255 * 256 = 65 280.
 *               2 * 64 * e_c + 16 K <= 128 * 56 100 + 4096 = 7 184 896 < 2^24.  S_c <= 255 * 256 = 65 280 < 2^16, so S_c and K travel as
 *               16-bit fields.  Everything fits 32 bits, and the quotient's operands fit a float's 24 bits exactly.
 * The defaults -- amount_q4 = 16, coring_q4 = 8 (T = h / 2: at +-6 uniform noise and h = 12 that is 6, about twice the standard deviation of
 * the detail signal's noise), overshoot = 0, strength / fallback 12 -- are choices, not measurements.
 * 0 IS A VALUE of amount_q4 (the identity), coring_q4 (no coring) and overshoot (none), so the "0 means the default" convention of the other
 * stages does not hold for them: the primitives take the three raw, rsdsfm_sharpen_params_init sets the defaults, and a NULL params pointer
 * means them.  Only strength, scale, min_samples, band_min_samples and quantile_q8 keep "0: the default".
 * Measured on the definition (tests/test_sharpen_cpu.py, the quality scene: a flat third and an edge texture under a 3 x 3 binomial blur and
 * +-a noise, h = 2 a, eight seeds; mean absolute error against the clean frame as a ratio output / input): the textured part 0.695 - 0.699,
 * 0.832 - 0.839, 0.933 - 0.942 at a = 2, 6, 12 with the defaults and 0.632 - 0.635, 0.661 - 0.668, 0.716 - 0.727 without coring; the flat part
 * 1.0000 with the defaults and 1.243 - 1.258, 1.273 - 1.292, 1.275 - 1.291 without coring.  DESIGN.md section 12 ("Sharpen") has the scene, the
 * kernel, the LDS layout and the bytes.
 *
 * NOT here: deconvolution with an estimated point-spread function, radii other than the 5 x 5 binomial, a gain per brightness band,
 * sharpening inside the super-resolution's accumulate, Solver methods or package-level Python names (rsdsfm_sharpen.py is a module beside the
 * package), the fuzz campaign entry, the C++ mirror.
 */
#ifndef RSDSFM_SHARPEN_H
#define RSDSFM_SHARPEN_H

#include "rsdsfm_noise_curve.h"

#ifdef __cplusplus
extern "C" {
#endif

/* choices, not measurements */
#define RSDSFM_SHARPEN_AMOUNT_DEFAULT 16
#define RSDSFM_SHARPEN_CORING_DEFAULT 8
#define RSDSFM_SHARPEN_OVERSHOOT_DEFAULT 0
#define RSDSFM_SHARPEN_AMOUNT_MAX 64
#define RSDSFM_SHARPEN_CORING_MAX 64
#define RSDSFM_SHARPEN_OVERSHOOT_MAX 255

typedef struct rsdsfm_sharpen_params {
    int32_t amount_q4;    /* the gain in sixteenths, 0 .. 64; 0 is the identity, NOT a default */
    int32_t coring_q4;    /* the threshold as a fraction of h in sixteenths, 0 .. 64; 0 is no coring, NOT a default */
    int32_t overshoot;    /* how far the result may leave the local 3 x 3 range, 0 .. 255; 0 is none, NOT a default */
    int32_t strength;     /* h, or the fallback of the curve calls, 1 .. 255; 0: the default, 12 */
    int32_t struct_bytes; /* 0 or sizeof(rsdsfm_sharpen_params), as rsdsfm_sharpen_params_init sets it; anything else is refused */
    int32_t reserved[3];  /* 0; anything else is refused */
} rsdsfm_sharpen_params;

/* amount_q4 = 16, coring_q4 = 8, overshoot = 0, strength = 12, struct_bytes = sizeof.  A NULL params pointer means these values. */
int rsdsfm_sharpen_params_init(rsdsfm_sharpen_params* params);

/* The sharpened image as defined above, at one strength.  d_image: rows x cols x channels bytes; d_mask: rows x cols bytes; d_image_out: as
 * d_image; d_counts4_or_null: 4 int64 [unset, kept, sharpened, limited], 8-byte aligned, zeroed by a memset node on the context's stream in
 * front of the launch.  Every plane is on the DEVICE and 4-byte aligned; the outputs are distinct from the inputs and from each other (in-place
 * is refused: the kernel reads a halo of 2); every output byte is written, so the outputs need no preset.  rows, cols in [2, 16384].
 * amount_q4, coring_q4, overshoot: raw, 0 is a value; strength 1 .. 255 (0: 12).
 * One kernel launch (sharpen_kernel<CH, false>) on the context's stream; returns without waiting.
 * RSDSFM_ERR_INVALID with a "sharpen: ..." message and nothing enqueued: a NULL, misaligned or aliased pointer, channels, a size or a parameter
 * outside its range. */
int rsdsfm_sharpen_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols, int32_t amount_q4,
                       int32_t coring_q4, int32_t overshoot, int32_t strength, uint8_t* d_image_out, int64_t* d_counts4_or_null);

/* rsdsfm_sharpen_dev with the strength per pixel from a curve: d_curve36 (36 uint64 on the DEVICE, 8-byte aligned, only read:
 * rsdsfm_noise_curve_dev's curve), scale, min_samples and band_min_samples as rsdsfm_denoise_spatial_curve_dev takes them; `strength` is the
 * fallback.  Every workgroup forms the 256-entry table in LDS itself; a pixel's strength is the entry at its own level.  With row 8 below
 * min_samples every byte is rsdsfm_sharpen_dev's at the fallback; with a flat curve every byte is rsdsfm_sharpen_dev's at
 * rsdsfm_noise_strength(n, m, scale, strength, min_samples).  One kernel launch (sharpen_kernel<CH, true>).
 * RSDSFM_ERR_INVALID ("sharpen curve: ..."): rsdsfm_sharpen_dev's list, a NULL, misaligned or aliased d_curve36, scale outside [0, 255],
 * min_samples < 0, band_min_samples < 0. */
int rsdsfm_sharpen_curve_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols, int32_t amount_q4,
                             int32_t coring_q4, int32_t overshoot, int32_t strength, const uint64_t* d_curve36, int32_t scale, int64_t min_samples,
                             int64_t band_min_samples, uint8_t* d_image_out, int64_t* d_counts4_or_null);

/* Kernel launches of rsdsfm_sharpen_dev and of rsdsfm_sharpen_curve_dev: 1.  The memset of the counters is not counted.  Host only. */
int rsdsfm_sharpen_launches(void);

/* Any 8-bit image under a mask measured and sharpened: rsdsfm_noise_curve_dev on the input with curve->quantile_q8, then
 * rsdsfm_sharpen_curve_dev on that curve with params' four words and curve's scale, min_samples and band_min_samples.  d_curve36_or_null: 36
 * DEVICE uint64, 8-byte aligned: the frame's curve, none of the other planes; NULL: the curve stays in the workspace.  The histogram (32 KB)
 * and a curve join the dense workspace with the first call, as the noise-curve frame call's do, and are released by rsdsfm_destroy.  Every
 * output is byte for byte the two public calls made one after another; whatever either would refuse is refused before the first enqueue.
 * Returns without waiting.
 * RSDSFM_ERR_INVALID ("sharpen frame: ...", or the parameter structs' own messages): both calls' lists, a non-zero reserved word, a
 * struct_bytes that is neither 0 nor sizeof. */
int rsdsfm_sharpen_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols,
                             const rsdsfm_sharpen_params* params_or_null, const rsdsfm_noise_curve_params* curve_params_or_null, uint8_t* d_image_out,
                             int64_t* d_counts4_or_null, uint64_t* d_curve36_or_null);

/* Kernel launches of rsdsfm_sharpen_frame_dev: 3 = rsdsfm_noise_curve_launches() + rsdsfm_sharpen_launches().  Host only. */
int rsdsfm_sharpen_frame_launches(void);

/* rsdsfm_sharpen_frame_dev per frame of a clip of images: d_images, d_masks, d_out_images: HOST arrays of nframes DEVICE pointers (nframes in
 * [1, 4096]); no solved clip is needed.  counts_or_null: HOST, nframes x 4 int64; curves_or_null: HOST, nframes x 36 uint64, every frame's
 * curve.  With either the call ends with one copy and one wait (the frames' 40 device words live in a buffer the call allocates and frees);
 * without both it only enqueues, every frame's curve in the workspace.  Every frame is checked before the first enqueue.
 * RSDSFM_ERR_INVALID ("sharpen video: ..."): a NULL array or entry, nframes outside its range, an output that is an input of ANY frame or
 * another frame's output, and the frame call's list. */
int rsdsfm_sharpen_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, const uint8_t* const* d_masks, int32_t nframes, int32_t channels, int32_t rows,
                             int32_t cols, const rsdsfm_sharpen_params* params_or_null, const rsdsfm_noise_curve_params* curve_params_or_null,
                             uint8_t* const* d_out_images, int64_t* counts_or_null, uint64_t* curves_or_null);

#ifdef __cplusplus
}
#endif

#endif /* RSDSFM_SHARPEN_H */
