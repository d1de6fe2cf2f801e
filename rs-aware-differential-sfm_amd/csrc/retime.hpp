// retime.hpp -- the retimer (include/rsdsfm_retime.h): what retime_kernels.hip and retime_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_retime.h"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {

constexpr int kRetimeWeightMax = 65535, kRetimeThresholdMax = 255;
constexpr int kRetimeGridMax = 1024;  // workgroups of the merge: 5 atomics each at most

// DenseWs::d_layer2, the retimer's layer B: [mask: P][image: 3 P], P = blend_plane_bytes (layer A is the blend's layer, stabilize_blend.hpp)
inline size_t retime_layer2_bytes(int rows, int cols) { return 4 * blend_plane_bytes(rows, cols); }

// the merge on c->stream (arguments checked by the caller; d_image_b and d_mask_b both NULL: b absent everywhere): the counters zeroed by a
// memset when passed, then one launch
int retime_merge_launch(Ctx* c, const unsigned char* d_image_a, const unsigned char* d_mask_a, const unsigned char* d_image_b, const unsigned char* d_mask_b,
                        int channels, int rows, int cols, int weight_q16, int threshold, unsigned char* d_image_out, unsigned char* d_mask_out,
                        unsigned char* d_source, int64_t* d_counts5);

}  // namespace rsdsfm
