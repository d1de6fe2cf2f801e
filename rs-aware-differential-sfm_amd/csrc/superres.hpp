// superres.hpp -- the multi-frame super-resolution (include/rsdsfm_superres.h): what superres_kernels.hip and superres_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_superres.h"
#include "denoise.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {

constexpr int kSuperresScaleMax = RSDSFM_SUPERRES_SCALE_MAX, kSuperresScaleDefault = RSDSFM_SUPERRES_SCALE_DEFAULT;
constexpr int kSuperresRadiusMax = RSDSFM_SUPERRES_RADIUS_MAX, kSuperresRadiusDefault = RSDSFM_SUPERRES_RADIUS_DEFAULT;
constexpr int kSuperresLayersMax = RSDSFM_SUPERRES_LAYERS_MAX;  // 16 (1 + 14) = 240 and 240 * 255 = 61 200 < 65 536: a uint16 sum cannot overflow
constexpr int kSuperresSourcesMax = 1 + kSuperresLayersMax;
constexpr int kSuperresStrengthDefault = RSDSFM_SUPERRES_STRENGTH_DEFAULT, kSuperresStrengthMax = 255;
constexpr unsigned kSuperresProxMax = RSDSFM_SUPERRES_PROX_MAX;  // = kDenoiseW: the own frame's nearest sample counts at most 16
constexpr int kSuperresSizeMax = 16384;

// DenseWs::d_superres, P = blend_plane_bytes of the FINE size (a multiple of 8, so the cells and the record are 8-byte aligned):
// [own prox: P][own validity: P][own bil: 3 P][own near: 3 P][layer prox: P][layer bil: 3 P][layer near: 3 P][cells: 8 P][one record: 8 uint64]
inline size_t superres_ws_bytes(int orows, int ocols) { return 23 * blend_plane_bytes(orows, ocols) + 8 * sizeof(uint64_t); }

// one source onto the fine grid on c->stream (arguments checked by the caller; iterations 1 .. 16): the dense rectifier's stage A, the
// stabiliser's map kernel with vp -- both on the source grid, as stabilize_window_launch enqueues them -- and superres_warp_kernel<CH>
int superres_render_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img, int channels, const double* d_depth_cm, const double* d_R, const double* d_t, double fx,
                           double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp, int scale, const int32_t window[4],
                           unsigned char* d_bil, unsigned char* d_near, unsigned char* d_prox, unsigned char* d_valid);

// one step on c->stream (arguments checked by the caller; the three layer planes all NULL: no layer; d_sums NULL: no gain): the counters zeroed
// by a memset when passed and `last`, then one launch
int superres_accumulate_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rnear, const unsigned char* d_rprox, const unsigned char* d_layer,
                               const unsigned char* d_lnear, const unsigned char* d_lprox, int channels, int rows, int cols, const unsigned long long* d_sums,
                               int64_t min_overlap, int gain_mode, int strength, uint16_t* d_cells, bool first, bool last, unsigned char* d_image_out,
                               unsigned char* d_mask_out, unsigned char* d_weight, int64_t* d_counts3);

}  // namespace rsdsfm
