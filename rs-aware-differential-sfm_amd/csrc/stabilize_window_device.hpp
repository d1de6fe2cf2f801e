// stabilize_window_device.hpp -- stage C with the target given (include/rsdsfm_stabilize_crop.h; tests/stabilize_crop_spec_numpy.py): the
// fixed point about a target, the sample there, and the window's targets -- what the window-warp kernels (stabilize_crop_kernels.hip) and
// the occlusion test's warp kernels (stabilize_visible_kernels.hip) share.  float64, one rounding per operation (-ffp-contract=off).
#pragma once

#include "rectify_dense_device.hpp"

namespace rsdsfm {

namespace {

// p = t, p <- t - D(p); returns the validity of p
__device__ __forceinline__ bool warp_fixed_point(const float2* __restrict__ disp, int rows, int cols, int iterations, double gx, double gy, double& px, double& py) {
    px = gx, py = gy;
    for (int it = 0; it < iterations; ++it) {
        const Tap tx = tap(px, cols), ty = tap(py, rows);
        const float2* r0 = disp + (int64_t)ty.i0 * cols;
        const float2* r1 = disp + (int64_t)ty.i1 * cols;
        const float2 d00 = r0[tx.i0], d01 = r0[tx.i1], d10 = r1[tx.i0], d11 = r1[tx.i1];
        const double dx = lerp(lerp((double)d00.x, (double)d01.x, tx.a), lerp((double)d10.x, (double)d11.x, tx.a), ty.a);
        const double dy = lerp(lerp((double)d00.y, (double)d01.y, tx.a), lerp((double)d10.y, (double)d11.y, tx.a), ty.a);
        px = gx - dx;
        py = gy - dy;
    }
    return px >= -0.5 && px < (double)cols - 0.5 && py >= -0.5 && py < (double)rows - 0.5;  // false for NaN / inf
}

// v[CH] = the image at taps (tx, ty), 0 where not valid
template <int CH>
__device__ __forceinline__ void warp_sample(const unsigned char* __restrict__ img, int cols, const Tap& tx, const Tap& ty, bool valid, unsigned* v) {
    const unsigned char* r0 = img + ((int64_t)ty.i0 * cols) * CH;
    const unsigned char* r1 = img + ((int64_t)ty.i1 * cols) * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const double i00 = (double)r0[tx.i0 * CH + c], i01 = (double)r0[tx.i1 * CH + c], i10 = (double)r1[tx.i0 * CH + c], i11 = (double)r1[tx.i1 * CH + c];
        const unsigned s = saturate_u8(lerp(lerp(i00, i01, tx.a), lerp(i10, i11, tx.a), ty.a));
        v[c] = valid ? s : 0u;
    }
}

// warp_pixel (rectify_dense_device.hpp) with the target given: the fixed point about (gx, gy), then the sample
template <int CH>
__device__ __forceinline__ unsigned warp_pixel_at(const unsigned char* __restrict__ img, const float2* __restrict__ disp, int rows, int cols, int iterations,
                                                  double gx, double gy, unsigned* v) {
    double px, py;
    const bool valid = warp_fixed_point(disp, rows, cols, iterations, gx, gy, px, py);
    warp_sample<CH>(img, cols, tap(px, cols), tap(py, rows), valid, v);
    return valid ? 1u : 0u;
}

// the window (r0, c0) and the scales sy = h / rows, sx = w / cols, as doubles: uniform
struct CropMap {
    double r0, c0, sy, sx;
};

// the target of output pixel p of the full-size frame, mapped into the window
__device__ __forceinline__ void window_target(const CropMap& wm, int cols, int p, double& tx, double& ty) {
    const int iy = p / cols, ix = p - iy * cols;
    tx = (wm.c0 + ((double)ix + 0.5) * wm.sx) - 0.5;
    ty = (wm.r0 + ((double)iy + 0.5) * wm.sy) - 0.5;
}

}  // namespace

}  // namespace rsdsfm
