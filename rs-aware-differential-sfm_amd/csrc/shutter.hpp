// shutter.hpp -- the synthetic shutter (include/rsdsfm_shutter.h): what shutter_kernels.hip and shutter_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_shutter.h"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {

constexpr int kShutterSamplesMax = RSDSFM_SHUTTER_SAMPLES_MAX;  // 64 * 255 = 16 320 < 65 536: a uint16 sum cannot overflow
constexpr int kShutterGridMax = 1024;                           // workgroups of the accumulate: 3 atomics each at most

// DenseWs::d_shutter: [sample mask: P][sample image: 3 P][cells: 8 P], P = blend_plane_bytes (a multiple of 8, so the cells are 8-byte aligned);
// apart from layers A and B, which the retime frame call renders onto while the cells hold the sums
inline size_t shutter_ws_bytes(int rows, int cols) { return 12 * blend_plane_bytes(rows, cols); }

// one sample on c->stream (arguments checked by the caller): the counters zeroed by a memset when passed and `last`, then one launch
int shutter_accumulate_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, int channels, int rows, int cols, uint16_t* d_cells, bool first, bool last,
                              int nsamples, int min_samples, unsigned char* d_image_out, unsigned char* d_mask_out, unsigned char* d_coverage, int64_t* d_counts3);

}  // namespace rsdsfm
