// stabilize_inpaint.hpp -- the stabiliser's inpainting (include/rsdsfm_stabilize_inpaint.h): what stabilize_inpaint_kernels.hip and
// stabilize_inpaint_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

// tests/stabilize_inpaint_spec_numpy.py's constant
constexpr unsigned kSourceInpainted = 255u;

// DenseWs::d_inpaint: the levels 1 .. top of rectify_dense_plan(rows, cols), one 8-byte cell each, then one 8-byte slot whose first word says
// whether the 1 x 1 level is valid
inline size_t inpaint_ws_bytes(int rows, int cols) { return 8u * (rectify_dense_plan(rows, cols).total + 1u); }

// kernel launches of one frame: level 0 -> 1, the large pulls, the single-workgroup launch, the large pushes, the output
int inpaint_launch_count(int rows, int cols);

// the launches of one frame on c->stream (arguments checked by the caller); d_pyr: inpaint_ws_bytes(rows, cols) bytes, 8-byte aligned
int inpaint_launch(Ctx* c, void* d_pyr, unsigned char* d_image, const unsigned char* d_mask, int channels, int rows, int cols, unsigned char* d_source,
                   int64_t* d_count);

}  // namespace rsdsfm
