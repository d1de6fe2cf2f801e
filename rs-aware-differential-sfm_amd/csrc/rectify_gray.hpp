// rectify_gray.hpp -- the one-channel rectifier (rectify_kernels.hip) as its C ABI (rectify_host.hip, rectify_video_host.hip) launches it.
#pragma once

#include <stdint.h>

#include "rsdsfm_internal.hpp"

namespace rsdsfm {

// rectify_frame_launch on gray images: d_img, d_gs, d_fixed are rows x cols bytes; a value g stands for the BGR pixel (g, g, g) and the
// outputs are channel 0 of rectify_frame_launch's for that image; d_preview and d_c3d are its, bit for bit.  d_partials: >= 2 * 1024 doubles
int rectify_gray_frame_launch(Ctx* c, const double* d_inl, int64_t m, const unsigned char* d_img, const double* d_depth_cm, const double* d_R,
                              const double* d_t, double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int offset,
                              unsigned char* d_preview, unsigned char* d_gs, float* d_c3d, unsigned char* d_fixed, double* d_partials);

}  // namespace rsdsfm
