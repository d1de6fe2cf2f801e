// deblur.hpp -- the sharpness transfer (include/rsdsfm_deblur.h): what deblur_kernels.hip and deblur_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_deblur.h"
#include "denoise.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

constexpr int kDeblurRadiusMax = RSDSFM_DEBLUR_RADIUS_MAX;
constexpr int kDeblurLayersMax = RSDSFM_DEBLUR_LAYERS_MAX;
constexpr int kDeblurSourcesMax = 1 + kDeblurLayersMax;
constexpr int kDeblurStrengthDefault = RSDSFM_DEBLUR_STRENGTH_DEFAULT, kDeblurStrengthMax = 255;
constexpr int kDeblurMarginDefault = RSDSFM_DEBLUR_MARGIN_DEFAULT, kDeblurMarginMax = RSDSFM_DEBLUR_MARGIN_MAX;
constexpr int64_t kDeblurMinPairsDefault = RSDSFM_DEBLUR_MIN_PAIRS_DEFAULT;
constexpr unsigned kDeblurTauMax = RSDSFM_DEBLUR_TAU_MAX;
constexpr int kDeblurBandsMax = RSDSFM_DEBLUR_BANDS_MAX;
constexpr int kDeblurBandRowsMin = 16, kDeblurBandRowsMax = 16384;  // a multiple of the tile's 16 rows: a tile then lies in one band
constexpr unsigned kDeblurBias = 765u;  // Y_R - Y_L + bias lies in [0, 1530]
// 16 (the own frame) + 7 * 32 = 240 = 16 (1 + 14): the cells' bounds are the denoise's
static_assert(kDenoiseW + kDeblurLayersMax * kDeblurTauMax <= kDenoiseW * (1 + kDenoiseLayersMax), "a uint16 sum cannot overflow");

// the ABI's margin word as its value: -1 none, 0 the default
inline int deblur_margin_value(int word) { return word < 0 ? 0 : word == 0 ? kDeblurMarginDefault : word; }

// tau of the record T = [pairs, A_R, A_L, 0]: the spec's tau(); host and device.  margin: the value, 0 .. 64; min_pairs >= 1.
// A <= 2 * 16384^2 * 765^2 < 2^49, so 80 A < 2^56: nothing overflows
__host__ __device__ inline unsigned deblur_tau_of(const unsigned long long* T, int margin, long long min_pairs) {
    const unsigned long long ar = T[1], al = T[2];
    if ((long long)T[0] < min_pairs || 16ull * al <= (16ull + (unsigned long long)margin) * ar) return 0u;
    const unsigned long long q = (16ull * (al - ar)) / (ar ? ar : 1ull);
    return q > kDeblurTauMax ? kDeblurTauMax : (unsigned)q;
}

// band_rows as the band calls take it: a multiple of 16 in [16, 16384]
inline bool deblur_band_rows_ok(int band_rows) { return band_rows >= kDeblurBandRowsMin && band_rows <= kDeblurBandRowsMax && band_rows % kDeblurBandRowsMin == 0; }
inline int deblur_bands_of(int rows, int band_rows) { return (rows + band_rows - 1) / band_rows; }

// tau of row y, the spec's row_taus(): b = y / H the row's band, tb its tau, ta and tc those of the bands above and below (of band b itself at
// the frame's ends; they are not used there).  Band centres c_b = b H + H / 2; tb in front of the first and from the last centre on, else
// linear between the two centres about y, rounded half up.  <= 32 * 16384 + 8192: nothing overflows.  Host and device.
__host__ __device__ inline unsigned deblur_row_tau_of(int y, int b, int H, int nbands, unsigned ta, unsigned tb, unsigned tc) {
    const int h2 = H / 2;
    if (y < h2 || y >= (nbands - 1) * H + h2) return tb;
    const int lo = (y - h2) / H;  // b - 1 or b
    const unsigned f = (unsigned)((y - h2) - lo * H), uh = (unsigned)H;
    const unsigned t0 = lo == b ? tb : ta, t1 = lo == b ? tc : tb;
    return (t0 * (uh - f) + t1 * f + (unsigned)h2) / uh;
}

// the record zeroed by a memset, then one launch, on c->stream (arguments checked by the caller; d_sums NULL: no gain)
int deblur_sharpness_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                            int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, unsigned long long* d_sharp4);

// one step on c->stream (arguments checked by the caller; d_layer, d_lmask and d_sharp all NULL: no layer; margin: the value): the counters
// zeroed by a memset when passed and `last`, then one launch
int deblur_accumulate_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                             int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int strength, const unsigned long long* d_sharp4,
                             int margin, int64_t min_pairs, int gate_mode, uint16_t* d_cells, bool first, bool last, unsigned char* d_image_out, unsigned char* d_mask_out,
                             unsigned char* d_weight, int64_t* d_counts3);

// deblur_bands_kernels.hip: the same two with a record per band of band_rows rows (nbands = ceil(rows / band_rows) records of 4 words)
int deblur_band_sharpness_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                                 int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int band_rows, unsigned long long* d_records);
int deblur_band_accumulate_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                                  int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int strength,
                                  const unsigned long long* d_records, int band_rows, int margin, int64_t min_pairs, int gate_mode, uint16_t* d_cells, bool first, bool last,
                                  unsigned char* d_image_out, unsigned char* d_mask_out, unsigned char* d_weight, int64_t* d_counts3);

}  // namespace rsdsfm
