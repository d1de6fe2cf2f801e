// stabilize.hpp -- the stabiliser (include/rsdsfm_stabilize.h): what stabilize_kernels.hip and stabilize_host.hip share.
#pragma once

#include <stdint.h>

#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

// the virtual pose of one frame, a kernel argument: X_virtual = M X_first_scanline + m (M row-major)
struct StabPose {
    double M[9];
    double m[3];
};

// the launches of one frame on c->stream (arguments checked by the caller; iterations 1 .. 16): the dense rectifier's stage A, the
// stabiliser's map kernel, the dense rectifier's stage C and, when d_valid is set, the count of d_mask (then not NULL)
int stabilize_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img, int channels, const double* d_depth_cm, const double* d_R, const double* d_t, double fx,
                     double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp, unsigned char* d_out,
                     unsigned char* d_mask, double* d_filled_cm, int64_t* d_valid);

}  // namespace rsdsfm
