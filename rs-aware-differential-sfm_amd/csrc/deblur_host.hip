// deblur_host.hip -- C ABI of the sharpness transfer (include/rsdsfm_deblur.h; tests/deblur_spec_numpy.py is the definition,
// deblur_kernels.hip the kernels): the sharpness call, the host-only tau, the accumulate call, the frame call, which CALLS the public render
// entry points, the overlap record, the sharpness call and the accumulate one after another on the denoise's planes of the context's dense
// workspace, and the clip call, which calls the frame call per frame (walk_clip, clip_stage_host.hpp).  The calls per scanline band
// (tests/deblur_bands_spec_numpy.py, deblur_bands_kernels.hip) share every check with the calls they stand beside.
#include <vector>

#include "clip_stage_host.hpp"
#include "deblur.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {
namespace {

rsdsfm_deblur_params deblur_defaults() {
    return rsdsfm_deblur_params{RSDSFM_DEBLUR_RADIUS_DEFAULT, kDeblurStrengthDefault, kDeblurMarginDefault, 0, 0, 0, 0, (int32_t)sizeof(rsdsfm_deblur_params),
                                kMinOverlapDefault,           kDeblurMinPairsDefault, 0, {0, 0, 0}};
}

bool margin_word_ok(int margin) { return margin >= -1 && margin <= kDeblurMarginMax; }

// the params with every 0 of radius, strength, margin, min_overlap and min_pairs replaced by its default (the margin stays the ABI's word: -1
// is "none"), or the defaults for NULL; false: refused
bool deblur_params_resolve(const rsdsfm_deblur_params* in, rsdsfm_deblur_params* out) {
    *out = in ? *in : deblur_defaults();
    if (!struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_deblur_params))) return false;
    if (out->radius == 0) out->radius = RSDSFM_DEBLUR_RADIUS_DEFAULT;
    if (out->strength == 0) out->strength = kDeblurStrengthDefault;
    if (out->margin == 0) out->margin = kDeblurMarginDefault;
    if (out->min_overlap == 0) out->min_overlap = kMinOverlapDefault;
    if (out->min_pairs == 0) out->min_pairs = kDeblurMinPairsDefault;
    return out->radius >= 1 && out->radius <= kDeblurRadiusMax && out->strength >= 1 && out->strength <= kDeblurStrengthMax && margin_word_ok(out->margin) &&
           (out->gate_mode == 0 || out->gate_mode == 1) && out->min_overlap >= 0 && out->min_pairs >= 0 && (out->gain_mode == 0 || out->gain_mode == 1) &&
           occlusion_words_ok(out->occlusion, out->occlusion_tol_q16);
}

const char* const kDeblurParamsMessage =
    "rsdsfm_deblur_params: radius in [1, 3] or 0, strength in [1, 255] or 0, margin in [-1, 64], gate_mode 0 or 1, gain_mode 0 or 1, occlusion 0 or 1, "
    "occlusion_tol_q16 in [0, 65536], min_overlap >= 0, min_pairs >= 0, struct_bytes 0 or sizeof (use rsdsfm_deblur_params_init)";

// band_rows and the bands it gives: new texts, the params' message above stays as it is
const char* const kDeblurBandRowsMessage = "deblur bands: band_rows must be a multiple of 16 in [16, 16384]";
const char* const kDeblurBandCountMessage = "deblur bands: rows / band_rows gives more than 64 bands (RSDSFM_DEBLUR_BANDS_MAX)";
const char* const kDeblurParamsBandRowsMessage = "rsdsfm_deblur_params: band_rows must be 0 (off) or a multiple of 16 in [16, 16384]";

// rows in [2, 16384] already
int band_rows_check(Ctx* c, int rows, int band_rows) {
    if (!deblur_band_rows_ok(band_rows)) return fail(c, RSDSFM_ERR_INVALID, kDeblurBandRowsMessage);
    if (deblur_bands_of(rows, band_rows) > kDeblurBandsMax) return fail(c, RSDSFM_ERR_INVALID, kDeblurBandCountMessage);
    return RSDSFM_OK;
}

// the checks of the two sharpness calls, behind the context's: the size, the knobs, the planes and the record(s)
int sharpness_check(Ctx* c, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image, const uint8_t* d_layer_mask, int32_t channels, int32_t rows,
                    int32_t cols, const uint64_t* d_sums8_or_null, int64_t min_overlap, int32_t gain_mode, const uint64_t* d_out) {
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "deblur sharpness: rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "deblur sharpness: channels must be 1 or 3");
    if (min_overlap < 0 || (gain_mode != 0 && gain_mode != 1)) return fail(c, RSDSFM_ERR_INVALID, "deblur sharpness: min_overlap must be >= 0 and gain_mode 0 or 1");
    if (!d_ref_image || !d_ref_mask || !d_layer_image || !d_layer_mask || !d_out) return fail(c, RSDSFM_ERR_INVALID, "deblur sharpness: null device pointer");
    if (((uintptr_t)d_ref_image | (uintptr_t)d_ref_mask | (uintptr_t)d_layer_image | (uintptr_t)d_layer_mask) & 3u)
        return fail(c, RSDSFM_ERR_INVALID, "deblur sharpness: every plane must be 4-byte aligned");
    if (((uintptr_t)d_out | (uintptr_t)d_sums8_or_null) & 7u) return fail(c, RSDSFM_ERR_INVALID, "deblur sharpness: the records must be 8-byte aligned");
    const void* in[5] = {d_ref_image, d_ref_mask, d_layer_image, d_layer_mask, d_sums8_or_null};
    for (int i = 0; i < 5; ++i) {
        if (in[i] == (const void*)d_out) return fail(c, RSDSFM_ERR_INVALID, "deblur sharpness: the record may not be an input");
        for (int j = i + 1; j < 4; ++j)
            if (in[i] == in[j]) return fail(c, RSDSFM_ERR_INVALID, "deblur sharpness: the reference's and the layer's planes must be distinct");
    }
    return RSDSFM_OK;
}

// the denoise's reference planes and cells and the blend's layer, made when first asked for, and this stage's one record
int deblur_ws(Ctx* c, int rows, int cols, DenseWs** ws) {
    int rc = rectify_dense_ws(c, rows, cols, ws);  // a size change releases them with the rest
    if (rc != RSDSFM_OK) return rc;
    rc = ensure_plane(c, &(*ws)->d_layer, blend_layer_bytes(rows, cols), "deblur: no memory for the layer");
    if (rc != RSDSFM_OK) return rc;
    rc = ensure_plane(c, &(*ws)->d_denoise, denoise_ws_bytes(rows, cols), "deblur: no memory for the reference planes and the cells");
    if (rc != RSDSFM_OK) return rc;
    return ensure_plane(c, &(*ws)->d_deblur, 4 * sizeof(unsigned long long), "deblur: no memory for the sharpness record");
}

// the band records' own plane, of a fixed size (ensure_plane does not track sizes): 64 records
int deblur_bands_ws(Ctx* c, DenseWs* ws) {
    return ensure_plane(c, &ws->d_deblur_bands, (size_t)kDeblurBandsMax * 4 * sizeof(unsigned long long), "deblur: no memory for the band records");
}

static_assert(kDeblurSourcesMax <= kClipSourcesMax, "a frame's sources fit a ClipPlan");
constexpr int kDeblurTausPerFrame = 2 * kDeblurRadiusMax;           // 6
// the counters, then the records of nbands bands per neighbour, as int64
constexpr int deblur_words_per_frame(int nbands) { return 3 + 4 * kDeblurTausPerFrame * nbands; }

// both accumulate calls: band_rows 0 is the call with one record
int accumulate_call(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image_or_null, const uint8_t* d_layer_mask_or_null,
                    int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null, int64_t min_overlap, int32_t gain_mode, int32_t strength,
                    const uint64_t* d_sharp_or_null, bool bands, int32_t band_rows, int32_t margin, int64_t min_pairs, int32_t gate_mode, uint16_t* d_cells_or_null,
                    int32_t first, int32_t last, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (min_overlap < 0 || (gain_mode != 0 && gain_mode != 1) || strength < 0 || strength > kDeblurStrengthMax)
        return fail(c, RSDSFM_ERR_INVALID, "deblur accumulate: min_overlap must be >= 0, gain_mode 0 or 1 and strength in [1, 255] (0: the default, 24)");
    if (!margin_word_ok(margin) || min_pairs < 0 || (gate_mode != 0 && gate_mode != 1))
        return fail(c, RSDSFM_ERR_INVALID, "deblur accumulate: margin must be in [-1, 64], min_pairs >= 0 and gate_mode 0 or 1");
    if (d_layer_image_or_null && !d_sharp_or_null)
        return fail(c, RSDSFM_ERR_INVALID, bands ? "deblur accumulate: a layer needs its band records" : "deblur accumulate: a layer needs its sharpness record");
    if (!d_layer_image_or_null) d_sharp_or_null = nullptr, d_sums8_or_null = nullptr;  // not read
    AccumulateOutputs out{d_image_out, d_mask_out, d_weight_or_null, d_counts3_or_null};
    int rc = accumulate_check(c, "deblur", d_ref_image, d_ref_mask, d_layer_image_or_null, d_layer_mask_or_null, channels, rows, cols, d_cells_or_null,
                              {d_sums8_or_null, d_sharp_or_null}, first, last, &out);
    if (rc == RSDSFM_OK && bands) rc = band_rows_check(c, rows, band_rows);
    if (rc != RSDSFM_OK) return rc;
    const unsigned long long* sums = reinterpret_cast<const unsigned long long*>(d_sums8_or_null);
    const unsigned long long* sharp = reinterpret_cast<const unsigned long long*>(d_sharp_or_null);
    min_overlap = min_overlap ? min_overlap : kMinOverlapDefault;
    strength = strength ? strength : kDeblurStrengthDefault;
    min_pairs = min_pairs ? min_pairs : kDeblurMinPairsDefault;
    if (bands)
        return deblur_band_accumulate_launch(c, d_ref_image, d_ref_mask, d_layer_image_or_null, d_layer_mask_or_null, channels, rows, cols, sums, min_overlap, gain_mode,
                                             strength, sharp, band_rows, deblur_margin_value(margin), min_pairs, gate_mode, d_cells_or_null, first == 1, last == 1,
                                             out.image, out.mask, out.weight, out.counts);
    return deblur_accumulate_launch(c, d_ref_image, d_ref_mask, d_layer_image_or_null, d_layer_mask_or_null, channels, rows, cols, sums, min_overlap, gain_mode, strength,
                                    sharp, deblur_margin_value(margin), min_pairs, gate_mode, d_cells_or_null, first == 1, last == 1, out.image, out.mask, out.weight,
                                    out.counts);
}

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_deblur_params_init(rsdsfm_deblur_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = deblur_defaults();
    return RSDSFM_OK;
}

int rsdsfm_deblur_launches(int32_t rows, int32_t cols, int32_t nsrc) {
    if (nsrc < 1 || nsrc > kDeblurSourcesMax) return RSDSFM_ERR_INVALID;
    const int one = rsdsfm_stabilize_window_launches(rows, cols);
    if (one < 0) return one;
    return nsrc * one + (nsrc == 1 ? 1 : 3 * (nsrc - 1));
}

int rsdsfm_deblur_tau(const uint64_t* sharp4, int32_t margin, int64_t min_pairs, int32_t* tau_out) {
    if (!sharp4 || !tau_out || !margin_word_ok(margin) || min_pairs < 0) return RSDSFM_ERR_INVALID;
    const unsigned long long T[4] = {sharp4[0], sharp4[1], sharp4[2], sharp4[3]};
    *tau_out = (int32_t)deblur_tau_of(T, deblur_margin_value(margin), min_pairs ? min_pairs : kDeblurMinPairsDefault);
    return RSDSFM_OK;
}

int rsdsfm_deblur_sharpness_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image, const uint8_t* d_layer_mask,
                                int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null, int64_t min_overlap, int32_t gain_mode,
                                uint64_t* d_sharp4_out) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const int rc = sharpness_check(c, d_ref_image, d_ref_mask, d_layer_image, d_layer_mask, channels, rows, cols, d_sums8_or_null, min_overlap, gain_mode, d_sharp4_out);
    if (rc != RSDSFM_OK) return rc;
    return deblur_sharpness_launch(c, d_ref_image, d_ref_mask, d_layer_image, d_layer_mask, channels, rows, cols, reinterpret_cast<const unsigned long long*>(d_sums8_or_null),
                                   min_overlap ? min_overlap : kMinOverlapDefault, gain_mode, reinterpret_cast<unsigned long long*>(d_sharp4_out));
}

int rsdsfm_deblur_accumulate_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image_or_null,
                                 const uint8_t* d_layer_mask_or_null, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                                 int64_t min_overlap, int32_t gain_mode, int32_t strength, const uint64_t* d_sharp4_or_null, int32_t margin, int64_t min_pairs,
                                 int32_t gate_mode, uint16_t* d_cells_or_null, int32_t first, int32_t last, uint8_t* d_image_out, uint8_t* d_mask_out,
                                 uint8_t* d_weight_or_null, int64_t* d_counts3_or_null) {
    return accumulate_call(ctx, d_ref_image, d_ref_mask, d_layer_image_or_null, d_layer_mask_or_null, channels, rows, cols, d_sums8_or_null, min_overlap, gain_mode, strength,
                           d_sharp4_or_null, false, 0, margin, min_pairs, gate_mode, d_cells_or_null, first, last, d_image_out, d_mask_out, d_weight_or_null,
                           d_counts3_or_null);
}

int rsdsfm_deblur_band_sharpness_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image, const uint8_t* d_layer_mask,
                                     int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null, int64_t min_overlap, int32_t gain_mode,
                                     int32_t band_rows, uint64_t* d_band_records_out) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = sharpness_check(c, d_ref_image, d_ref_mask, d_layer_image, d_layer_mask, channels, rows, cols, d_sums8_or_null, min_overlap, gain_mode, d_band_records_out);
    if (rc == RSDSFM_OK) rc = band_rows_check(c, rows, band_rows);
    if (rc != RSDSFM_OK) return rc;
    return deblur_band_sharpness_launch(c, d_ref_image, d_ref_mask, d_layer_image, d_layer_mask, channels, rows, cols,
                                        reinterpret_cast<const unsigned long long*>(d_sums8_or_null), min_overlap ? min_overlap : kMinOverlapDefault, gain_mode, band_rows,
                                        reinterpret_cast<unsigned long long*>(d_band_records_out));
}

int rsdsfm_deblur_band_taus(const uint64_t* records, int32_t nbands, int32_t margin, int64_t min_pairs, int32_t* taus_out) {
    if (!records || !taus_out || nbands < 1 || nbands > kDeblurBandsMax) return RSDSFM_ERR_INVALID;
    for (int b = 0; b < nbands; ++b) {
        const int rc = rsdsfm_deblur_tau(records + 4 * b, margin, min_pairs, taus_out + b);
        if (rc != RSDSFM_OK) return rc;
    }
    return RSDSFM_OK;
}

int rsdsfm_deblur_row_taus(const int32_t* taus, int32_t nbands, int32_t band_rows, int32_t rows, int32_t* row_taus_out) {
    if (!taus || !row_taus_out || !deblur_band_rows_ok(band_rows) || !frame_size_ok(rows, rows) || nbands > kDeblurBandsMax || nbands != deblur_bands_of(rows, band_rows))
        return RSDSFM_ERR_INVALID;
    for (int b = 0; b < nbands; ++b)
        if (taus[b] < 0 || taus[b] > (int32_t)kDeblurTauMax) return RSDSFM_ERR_INVALID;
    for (int y = 0; y < rows; ++y) {
        const int b = y / band_rows;
        row_taus_out[y] = (int32_t)deblur_row_tau_of(y, b, band_rows, nbands, (unsigned)taus[b > 0 ? b - 1 : 0], (unsigned)taus[b], (unsigned)taus[b < nbands - 1 ? b + 1 : b]);
    }
    return RSDSFM_OK;
}

int rsdsfm_deblur_band_accumulate_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image_or_null,
                                      const uint8_t* d_layer_mask_or_null, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                                      int64_t min_overlap, int32_t gain_mode, int32_t strength, const uint64_t* d_band_records_or_null, int32_t band_rows,
                                      int32_t margin, int64_t min_pairs, int32_t gate_mode, uint16_t* d_cells_or_null, int32_t first, int32_t last,
                                      uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, int64_t* d_counts3_or_null) {
    return accumulate_call(ctx, d_ref_image, d_ref_mask, d_layer_image_or_null, d_layer_mask_or_null, channels, rows, cols, d_sums8_or_null, min_overlap, gain_mode, strength,
                           d_band_records_or_null, true, band_rows, margin, min_pairs, gate_mode, d_cells_or_null, first, last, d_image_out, d_mask_out, d_weight_or_null,
                           d_counts3_or_null);
}

int rsdsfm_deblur_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                            const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                            int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_deblur_params* params_or_null,
                            const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_weight_or_null, int64_t* d_counts3_or_null,
                            uint64_t* d_sharp_records_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc < 1 || nsrc > kDeblurSourcesMax) return fail(c, RSDSFM_ERR_INVALID, "deblur frame: nsrc must be in [1, 8]");
    rsdsfm_deblur_params dp;
    if (!deblur_params_resolve(params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDeblurParamsMessage);
    const bool bands = dp.band_rows != 0;
    if (bands && !deblur_band_rows_ok(dp.band_rows)) return fail(c, RSDSFM_ERR_INVALID, kDeblurParamsBandRowsMessage);
    if (bands && deblur_bands_of(rows, dp.band_rows) > kDeblurBandsMax) return fail(c, RSDSFM_ERR_INVALID, kDeblurBandCountMessage);
    const int nbands = bands ? deblur_bands_of(rows, dp.band_rows) : 1;
    rc = frame_sources_check(c, "deblur frame", d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, nsrc, {d_image_out, d_mask_out, d_weight_or_null});
    if (rc == RSDSFM_OK) rc = frame_poses_check(c, "deblur frame", M, m, nsrc);
    if (rc == RSDSFM_OK) rc = output_planes_check(c, "deblur", {d_image_out, d_mask_out, d_weight_or_null}, d_counts3_or_null, false);
    if (rc != RSDSFM_OK) return rc;
    if (((uintptr_t)d_sharp_records_or_null & 7u) ||
        (d_sharp_records_or_null && ((const void*)d_sharp_records_or_null == d_image_out || (const void*)d_sharp_records_or_null == d_mask_out ||
                                     (const void*)d_sharp_records_or_null == d_weight_or_null || (const void*)d_sharp_records_or_null == d_counts3_or_null)))
        return fail(c, RSDSFM_ERR_INVALID, "deblur frame: the sharpness records must be 8-byte aligned and no output");
    int32_t full[4];
    const int32_t* window = nullptr;
    rc = frame_window(c, "deblur frame", window_or_null, rows, cols, full, &window);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* ws = nullptr;
    rc = deblur_ws(c, rows, cols, &ws);
    if (rc == RSDSFM_OK && bands && !d_sharp_records_or_null) rc = deblur_bands_ws(c, ws);
    if (rc != RSDSFM_OK) return rc;
    const RenderGeom g{channels, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations};
    const DenoisePlanes r = denoise_planes(ws->d_denoise, rows, cols);
    const BlendLayer l = blend_layer(ws->d_layer, rows, cols);
    rc = render_reference(ctx, "deblur frame", source_view(d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, 0), g, M, m, window, r.rimage, r.rmask, r.rsource);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc == 1)
        return bands ? rsdsfm_deblur_band_accumulate_dev(ctx, r.rimage, r.rmask, nullptr, nullptr, channels, rows, cols, nullptr, dp.min_overlap, dp.gain_mode, dp.strength,
                                                         nullptr, dp.band_rows, dp.margin, dp.min_pairs, dp.gate_mode, nullptr, 1, 1, d_image_out, d_mask_out,
                                                         d_weight_or_null, d_counts3_or_null)
                     : rsdsfm_deblur_accumulate_dev(ctx, r.rimage, r.rmask, nullptr, nullptr, channels, rows, cols, nullptr, dp.min_overlap, dp.gain_mode, dp.strength, nullptr,
                                                    dp.margin, dp.min_pairs, dp.gate_mode, nullptr, 1, 1, d_image_out, d_mask_out, d_weight_or_null, d_counts3_or_null);
    for (int k = 1; k < nsrc; ++k) {
        rc = neighbour_step(ctx, "deblur frame: zeroing the layer failed", dp.occlusion == 1, dp.occlusion_tol_q16, source_view(d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, k),
                            g, M + 9 * k, m + 3 * k, window, r.rimage, r.rsource, l.image, l.mask, l.record);
        if (rc != RSDSFM_OK) return rc;
        uint64_t* sharp = d_sharp_records_or_null ? d_sharp_records_or_null + (size_t)4 * nbands * (k - 1) : reinterpret_cast<uint64_t*>(bands ? ws->d_deblur_bands : ws->d_deblur);
        rc = bands ? rsdsfm_deblur_band_sharpness_dev(ctx, r.rimage, r.rmask, l.image, l.mask, channels, rows, cols, l.record, dp.min_overlap, dp.gain_mode, dp.band_rows, sharp)
                   : rsdsfm_deblur_sharpness_dev(ctx, r.rimage, r.rmask, l.image, l.mask, channels, rows, cols, l.record, dp.min_overlap, dp.gain_mode, sharp);
        if (rc != RSDSFM_OK) return rc;
        rc = bands ? rsdsfm_deblur_band_accumulate_dev(ctx, r.rimage, r.rmask, l.image, l.mask, channels, rows, cols, l.record, dp.min_overlap, dp.gain_mode, dp.strength, sharp,
                                                       dp.band_rows, dp.margin, dp.min_pairs, dp.gate_mode, r.cells, k == 1, k == nsrc - 1, d_image_out, d_mask_out,
                                                       d_weight_or_null, d_counts3_or_null)
                   : rsdsfm_deblur_accumulate_dev(ctx, r.rimage, r.rmask, l.image, l.mask, channels, rows, cols, l.record, dp.min_overlap, dp.gain_mode, dp.strength, sharp,
                                                  dp.margin, dp.min_pairs, dp.gate_mode, r.cells, k == 1, k == nsrc - 1, d_image_out, d_mask_out, d_weight_or_null,
                                                  d_counts3_or_null);
        if (rc != RSDSFM_OK) return rc;
    }
    return RSDSFM_OK;
}

int rsdsfm_deblur_video_banded_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx,
                                   double fy, double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t,
                                   const double* A, const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode,
                                   int32_t iterations, const rsdsfm_deblur_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images,
                                   uint8_t* const* d_out_masks, uint8_t* const* d_out_weights_or_null, int64_t* counts_or_null, int32_t* taus_or_null,
                                   int32_t* band_taus_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    ClipOutputs outs;
    outs.planes[0] = d_out_images;
    outs.planes[1] = d_out_masks;
    outs.planes[2] = d_out_weights_or_null;
    int rc = clip_arrays_check(c, "deblur video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, outs, "its weight plane when the array is passed");
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_deblur_params dp;
    if (!deblur_params_resolve(params_or_null, &dp)) return fail(c, RSDSFM_ERR_INVALID, kDeblurParamsMessage);
    // the band count sizes the host's words, so band_rows and the size are looked at here too, with the frame call's texts
    if (dp.band_rows != 0 && !deblur_band_rows_ok(dp.band_rows)) return fail(c, RSDSFM_ERR_INVALID, kDeblurParamsBandRowsMessage);
    if (dp.band_rows != 0 && !frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "deblur video: rows and cols must be in [2, 16384]");
    if (dp.band_rows != 0 && deblur_bands_of(rows, dp.band_rows) > kDeblurBandsMax) return fail(c, RSDSFM_ERR_INVALID, kDeblurBandCountMessage);
    const int nbands = dp.band_rows != 0 ? deblur_bands_of(rows, dp.band_rows) : 1;
    const int words = deblur_words_per_frame(nbands);
    // per frame on the device [counts: 3][records: 6 x nbands x 4], copied to the host together: one copy and one wait
    const bool want = counts_or_null != nullptr || taus_or_null != nullptr || band_taus_or_null != nullptr;
    std::vector<int64_t> host(want ? (size_t)words * (size_t)nsources : 0);
    std::vector<int> listed((size_t)nsources, 0);  // the neighbours of every frame
    int q = 0;
    // the public entry point itself, so that it runs the code it runs alone
    rc = walk_clip(c, "deblur video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, dp.radius, outs, words, want ? host.data() : nullptr,
                   [&](const ClipFrame& f) {
                       listed[(size_t)q++] = f.plan->nsrc - 1;
                       return rsdsfm_deblur_frame_dev(ctx, f.img, channels, f.map, f.R, f.t, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, f.plan->nsrc, f.plan->M,
                                                      f.plan->m, params_or_null, window_or_null, f.out[0], f.out[1], f.out[2], f.d_counts,
                                                      f.d_counts ? reinterpret_cast<uint64_t*>(f.d_counts + 3) : nullptr);
                   });
    if (rc != RSDSFM_OK || !want) return rc;
    for (int f = 0; f < nsources; ++f) {
        const int64_t* w = host.data() + (size_t)words * (size_t)f;
        for (int k = 0; k < 3 && counts_or_null; ++k) counts_or_null[3 * f + k] = w[k];
        for (int j = 0; j < kDeblurTausPerFrame; ++j) {
            int32_t most = -1;
            for (int b = 0; b < nbands; ++b) {
                int32_t tau = -1;
                if (j < listed[(size_t)f]) (void)rsdsfm_deblur_tau(reinterpret_cast<const uint64_t*>(w + 3 + 4 * ((size_t)j * nbands + b)), dp.margin, dp.min_pairs, &tau);
                if (band_taus_or_null) band_taus_or_null[((size_t)kDeblurTausPerFrame * f + j) * nbands + b] = tau;
                if (tau > most) most = tau;
            }
            if (taus_or_null) taus_or_null[kDeblurTausPerFrame * f + j] = most;
        }
    }
    return RSDSFM_OK;
}

int rsdsfm_deblur_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                            double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                            const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                            const rsdsfm_deblur_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks,
                            uint8_t* const* d_out_weights_or_null, int64_t* counts_or_null, int32_t* taus_or_null) {
    return rsdsfm_deblur_video_banded_dev(ctx, d_frames, nsources, rows, cols, channels, fx, fy, cx, cy, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, mode, q5_mode,
                                          iterations, params_or_null, window_or_null, d_out_images, d_out_masks, d_out_weights_or_null, counts_or_null, taus_or_null, nullptr);
}

}  // extern "C"
