// denoise.hpp -- the temporal denoise (include/rsdsfm_denoise.h): what denoise_kernels.hip and denoise_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_denoise.h"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {

constexpr int kDenoiseRadiusMax = RSDSFM_DENOISE_RADIUS_MAX;
constexpr int kDenoiseLayersMax = RSDSFM_DENOISE_LAYERS_MAX;  // 16 (1 + 14) = 240 and 240 * 255 = 61 200 < 65 536: a uint16 sum cannot overflow
constexpr int kDenoiseSourcesMax = 1 + kDenoiseLayersMax;
constexpr int kDenoiseStrengthDefault = RSDSFM_DENOISE_STRENGTH_DEFAULT, kDenoiseStrengthMax = 255;
constexpr unsigned kDenoiseW = 16u;                        // the weight's scale: the own frame counts 16
constexpr int kDenoiseTileRows = 16, kDenoiseTileCols = 64;  // one workgroup's tile: kBP threads of 4 consecutive pixels of a row

// DenseWs::d_denoise: [reference mask: P][reference source: P][reference image: 3 P][cells: 8 P], P = blend_plane_bytes (a multiple of 8, so
// the cells are 8-byte aligned); apart from the blend's layer, which the neighbours are rendered onto while the cells hold the sums
inline size_t denoise_ws_bytes(int rows, int cols) { return 13 * blend_plane_bytes(rows, cols); }
struct DenoisePlanes {
    unsigned char *rmask, *rsource, *rimage;
    uint16_t* cells;
};
inline DenoisePlanes denoise_planes(unsigned char* d_denoise, int rows, int cols) {
    const size_t P = blend_plane_bytes(rows, cols);
    return DenoisePlanes{d_denoise, d_denoise + P, d_denoise + 2 * P, reinterpret_cast<uint16_t*>(d_denoise + 5 * P)};
}

// one step on c->stream (arguments checked by the caller; d_layer and d_lmask both NULL: no layer; d_sums NULL: no gain): the counters zeroed
// by a memset when passed and `last`, then one launch
int denoise_accumulate_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                              int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int strength, uint16_t* d_cells, bool first,
                              bool last, unsigned char* d_image_out, unsigned char* d_mask_out, unsigned char* d_weight, int64_t* d_counts3);

// the params with every 0 of radius, strength and min_overlap replaced by its default, or the defaults for NULL; false: refused, with
// kDenoiseParamsMessage (denoise_host.hip; the top-up's frame and clip calls refuse the temporal stage's params in the same words)
bool denoise_params_resolve(const rsdsfm_denoise_params* in, rsdsfm_denoise_params* out);
extern const char* const kDenoiseParamsMessage;

// the spatial top-up (rsdsfm_denoise_spatial_dev; denoise_spatial_kernels.hip, denoise_spatial_host.hip)
constexpr int kDenoiseSpatialTargetDefault = RSDSFM_DENOISE_SPATIAL_TARGET_DEFAULT, kDenoiseSpatialTargetMax = 255;
constexpr int kDenoiseSpatialSearchDefault = RSDSFM_DENOISE_SPATIAL_SEARCH_DEFAULT, kDenoiseSpatialSearchMax = RSDSFM_DENOISE_SPATIAL_SEARCH_MAX;

// DenseWs::d_denoise_spatial: [weight: P][image: 3 P], P = blend_plane_bytes: what the temporal stage writes for the top-up to read
inline size_t denoise_spatial_ws_bytes(int rows, int cols) { return 4 * blend_plane_bytes(rows, cols); }

// the top-up on c->stream (arguments checked and defaults resolved by the caller; d_weight, d_support, d_counts3 may be NULL): the counters
// zeroed by a memset when passed, then one launch
int denoise_spatial_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, const unsigned char* d_weight, int channels, int rows, int cols, int strength,
                           int target, int search, unsigned char* d_image_out, unsigned char* d_support, int64_t* d_counts3);

// the top-up's argument checks (denoise_spatial_host.hip), shared with the calls that take the strength from a noise record (noise_host.hip):
// every 0 replaced by its default, false: outside its range (kSpatialWordsMessage); the params likewise, or the defaults for NULL
// (kSpatialParamsMessage); what the primitive refuses about its planes, or NULL; the refusal itself, "<stage>: <what>"
bool spatial_words_resolve(int32_t* strength, int32_t* target, int32_t* search);
bool spatial_params_resolve(const rsdsfm_denoise_spatial_params* in, rsdsfm_denoise_spatial_params* out);
extern const char* const kSpatialWordsMessage;
extern const char* const kSpatialParamsMessage;
const char* spatial_planes_refusal(const uint8_t* d_image, const uint8_t* d_mask, const uint8_t* d_weight, int channels, int rows, int cols, const uint8_t* d_image_out,
                                   const uint8_t* d_support, const int64_t* d_counts3);
int spatial_fail(Ctx* c, const char* stage, const char* what);

}  // namespace rsdsfm
