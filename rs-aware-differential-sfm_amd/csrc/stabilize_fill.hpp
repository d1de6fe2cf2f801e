// stabilize_fill.hpp -- the stabiliser's border fill (include/rsdsfm_stabilize_fill.h): what stabilize_fill_kernels.hip and
// stabilize_fill_host.hip share.
#pragma once

#include <stdint.h>

#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize.hpp"

namespace rsdsfm {

// the stabiliser's map pass, DEFINED in stabilize_kernels.hip (which keeps its contents) and launched from stabilize_fill_kernels.hip too:
// both objects are linked into one library, so the launch goes through the defining unit's registration
__global__ void stabilize_map_kernel(const double* __restrict__ depth_cm, const double* __restrict__ lv1, int h1, int w1, const double* __restrict__ R,
                                     const double* __restrict__ t, double fx, double fy, double cx, double cy, double fyp, int rows, int cols, int mode, StabPose vp,
                                     float2* __restrict__ disp, double* __restrict__ filled_cm);

// the launches of one candidate on c->stream (arguments checked by the caller; iterations 1 .. 16): the dense rectifier's stage A, the
// stabiliser's map kernel with vp, and the fill-warp kernel in stage C's place: d_out / d_mask / d_source (may be NULL) are changed where
// d_mask is 0 and the candidate is valid; d_filled (may be NULL) is zeroed and receives the number of pixels taken
int stabilize_fill_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img_n, int channels, const double* d_depth_cm, const double* d_R, const double* d_t,
                          double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp, int source_id,
                          unsigned char* d_out, unsigned char* d_mask, unsigned char* d_source, int64_t* d_filled);

}  // namespace rsdsfm
