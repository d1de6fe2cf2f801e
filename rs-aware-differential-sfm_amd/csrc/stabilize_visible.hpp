// stabilize_visible.hpp -- the stabiliser's occlusion test (include/rsdsfm_stabilize_visible.h): what stabilize_visible_kernels.hip,
// stabilize_visible_host.hip and the clip loops that render neighbours (stabilize_fill_host.hip, stabilize_crop_host.hip,
// stabilize_blend_host.hip) share.
#pragma once

#include <stdint.h>

#include "../../include/rsdsfm_stabilize_visible.h"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize.hpp"

namespace rsdsfm {

constexpr int kVisibleTolQ16Max = 65536;
constexpr unsigned kZbufEmpty = 0x7f800000u;  // +inf: positive floats order as their bit patterns

// the two planes of the test (DenseWs::d_visible: [zv: rows x cols float][zbuf: rows x cols uint32])
struct VisibleWs {
    float* d_zv;
    unsigned* d_zbuf;
};
inline VisibleWs visible_ws_layout(void* d_visible, int rows, int cols) {
    float* zv = static_cast<float*>(d_visible);
    return VisibleWs{zv, reinterpret_cast<unsigned*>(zv + (size_t)rows * (size_t)cols)};
}
inline size_t visible_ws_bytes(int rows, int cols) { return 8 * (size_t)rows * (size_t)cols; }

// the two words of rsdsfm_stabilize_fill_params that ask for the test: occlusion 0 / 1, occlusion_tol_q16 0 (the default) .. 65536
inline bool visible_words_ok(const rsdsfm_stabilize_fill_params* fp) {
    return !fp || ((fp->occlusion == 0 || fp->occlusion == 1) && fp->occlusion_tol_q16 >= 0 && fp->occlusion_tol_q16 <= kVisibleTolQ16Max);
}
inline bool visible_asked(const rsdsfm_stabilize_fill_params* fp) { return fp && fp->occlusion == 1; }

// the launches of one frame through a window and the test on c->stream (arguments checked by the caller; iterations 1 .. 16; tol_q16
// 1 .. 65536): the dense rectifier's stage A, the 4-byte memset of zbuf, the map kernel that also writes zv and splats, and the warp kernel
// that tests and counts; as stabilize_window_launch otherwise
int stabilize_visible_launch(Ctx* c, const DenseWs& ws, const VisibleWs& vw, const unsigned char* d_img_n, int channels, const double* d_depth_cm, const double* d_R,
                             const double* d_t, double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp,
                             int source_id, const int32_t window[4], unsigned char* d_out, unsigned char* d_mask, unsigned char* d_source, int tol_q16,
                             int64_t* d_counts2);

}  // namespace rsdsfm
