// rectify_dense_device.hpp -- the device helpers of the dense global-shutter rectifier (rectify_dense_kernels.hip) that the stabiliser's
// map kernel (stabilize_kernels.hip) shares with it, as flow_device.hpp does for the flow kernels: tile geometry, inverse depth, lerp / tap,
// the pull and push cells, the splat's chain (split so that the point in the first scanline's coordinates is reachable) and the warp body.
// Everything is float64 with one rounding per operation (-ffp-contract=off); tests/rectify_dense_spec_numpy.py is the definition.
#pragma once

#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace rsdsfm {

namespace {

constexpr int kTX = 64;   // tile width (image columns) = one wave
constexpr int kTY = 16;   // tile height: 16 x 8 B = one 128-byte line of the column-major depth map per column
constexpr int kCB = 512;  // threads of the tile kernels: 8 waves x 2 scanlines
constexpr int kBP = 256;
constexpr int kSB = 1024;         // threads of the single-workgroup kernel
constexpr int kSmallCells = 8160; // its LDS, in doubles (with the level table just under the 64 KB a workgroup may take)

__device__ __forceinline__ unsigned char saturate_u8(double v) {  // rectify_kernels.hip's: cvRound (nearest even) + clamp
    const long long r = __double2ll_rn(v);
    return (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

// 1 / z of a valid depth (finite, positive, with a positive reciprocal), else 0
__device__ __forceinline__ double inverse_depth(double z) {
    const double r = 1.0 / z;
    return (z > 0.0 && z < INFINITY && r > 0.0) ? r : 0.0;
}

__device__ __forceinline__ double lerp(double a, double b, double t) { return a + t * (b - a); }

// position p on an axis of n samples, replicate border: NaN and -inf go to 0, +inf to n - 1
struct Tap {
    int i0, i1;
    double a;
};
__device__ __forceinline__ Tap tap(double p, int n) {
    const double lo = p > 0.0 ? p : 0.0;
    const double c = lo < (double)(n - 1) ? lo : (double)(n - 1);
    Tap t;
    t.i0 = (int)c;  // c >= 0: truncation is floor
    t.i1 = t.i0 + 1 < n - 1 ? t.i0 + 1 : n - 1;
    t.a = c - (double)t.i0;
    return t;
}

// the mean of the non-zero children, taken about the first of them (equal children give their value exactly); 0 if there is none
__device__ __forceinline__ double pull_cell(double c00, double c01, double c10, double c11) {
    const double a = c00 != 0.0 ? c00 : (c01 != 0.0 ? c01 : (c10 != 0.0 ? c10 : c11));
    const double d00 = c00 != 0.0 ? c00 - a : 0.0, d01 = c01 != 0.0 ? c01 - a : 0.0, d10 = c10 != 0.0 ? c10 - a : 0.0, d11 = c11 != 0.0 ? c11 - a : 0.0;
    const double s = ((d00 + d01) + d10) + d11;
    const int n = (c00 != 0.0) + (c01 != 0.0) + (c10 != 0.0) + (c11 != 0.0);
    return n > 0 ? a + s / (double)n : 0.0;
}

__device__ __forceinline__ double pull_from(const double* __restrict__ src, int hs, int ws, int X, int Y) {
    const int x0 = 2 * X, y0 = 2 * Y;
    const bool bx = x0 + 1 < ws, by = y0 + 1 < hs;
    const double* r0 = src + (int64_t)y0 * ws + x0;
    return pull_cell(r0[0], bx ? r0[1] : 0.0, by ? r0[ws] : 0.0, (bx && by) ? r0[ws + 1] : 0.0);
}

// what cell (x, y) of a level takes from the complete coarser level (hc x wc)
__device__ __forceinline__ double push_from(const double* __restrict__ lv, int hc, int wc, int x, int y) {
    const Tap tx = tap(((double)x + 0.5) * 0.5 - 0.5, wc), ty = tap(((double)y + 0.5) * 0.5 - 0.5, hc);
    const double* r0 = lv + (int64_t)ty.i0 * wc;
    const double* r1 = lv + (int64_t)ty.i1 * wc;
    return lerp(lerp(r0[tx.i0], r0[tx.i1], tx.a), lerp(r1[tx.i0], r1[tx.i1], tx.a), ty.a);
}

// RsFrame::backProject's chain for pixel (x, y) with depth z -- back_project_claim_body (rectify_kernels.hip) and rso_back_project
// (oracle/rsdsfm_oracle.c:2440-2458) operation for operation: planeToSpace, cameraToWorldFrame(Rr, tr), worldToCameraFrame(R0, t0), spaceToPlane.
// The splat's translation unit keeps its own copy (its bytes do not move); tests/test_rectify_dense_cpu.py holds the two together.
// rs_to_gs_point: the chain up to pg, the point in the coordinates of the first scanline's camera; rs_to_gs_project: spaceToPlane.
__device__ __forceinline__ void rs_to_gs_point(int x, int y, double z, const double* Rr, const double* tr, const double* R0, const double* t0, double fx, double fy,
                                               double cx, double cy, double* pg) {
    const double nx = ((double)x - cx) * 1.0 / fx;
    const double ny = ((double)y - cy) * 1.0 / fy;
    const double pc0 = z * nx, pc1 = z * ny, pc2 = z * 1.0;
    double pw[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double rt0 = Rr[i], rt1 = Rr[3 + i], rt2 = Rr[6 + i];  // row i of R^T
        const double ti = ((-rt0) * tr[0] + (-rt1) * tr[1]) + (-rt2) * tr[2];
        pw[i] = ((rt0 * pc0 + rt1 * pc1) + rt2 * pc2) + ti * 1.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) pg[i] = ((R0[i * 3] * pw[0] + R0[i * 3 + 1] * pw[1]) + R0[i * 3 + 2] * pw[2]) + t0[i] * 1.0;
}

__device__ __forceinline__ void rs_to_gs_project(const double* pg, double fx, double cx, double cy, double fyp, double& gx, double& gy) {
    gx = pg[0] / pg[2] * fx + cx;
    gy = pg[1] / pg[2] * fyp + cy;
}

__device__ __forceinline__ void rs_to_gs_chain(int x, int y, double z, const double* Rr, const double* tr, const double* R0, const double* t0, double fx, double fy,
                                               double cx, double cy, double fyp, double& gx, double& gy) {
    double pg[3];
    rs_to_gs_point(x, y, z, Rr, tr, R0, t0, fx, fy, cx, cy, pg);
    rs_to_gs_project(pg, fx, cx, cy, fyp, gx, gy);
}

// one output pixel: the fixed point, then the sample; v[CH] = the pixel, returns the mask
template <int CH>
__device__ __forceinline__ unsigned warp_pixel(const unsigned char* __restrict__ img, const float2* __restrict__ disp, int rows, int cols, int iterations, int p,
                                               unsigned* v) {
    const int iy = p / cols, ix = p - iy * cols;
    const double gx = (double)ix, gy = (double)iy;
    double px = gx, py = gy;
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
    const bool valid = px >= -0.5 && px < (double)cols - 0.5 && py >= -0.5 && py < (double)rows - 0.5;  // false for NaN / inf
    const Tap tx = tap(px, cols), ty = tap(py, rows);
    const unsigned char* r0 = img + ((int64_t)ty.i0 * cols) * CH;
    const unsigned char* r1 = img + ((int64_t)ty.i1 * cols) * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const double i00 = (double)r0[tx.i0 * CH + c], i01 = (double)r0[tx.i1 * CH + c], i10 = (double)r1[tx.i0 * CH + c], i11 = (double)r1[tx.i1 * CH + c];
        const unsigned s = saturate_u8(lerp(lerp(i00, i01, tx.a), lerp(i10, i11, tx.a), ty.a));
        v[c] = valid ? s : 0u;
    }
    return valid ? 1u : 0u;
}

// 4 output pixels (12 bytes = 3 dwords; one channel: one dword; mask: one dword) per thread
template <int CH>
__device__ __forceinline__ void warp_body(const unsigned char* __restrict__ img, const float2* __restrict__ disp, const double* __restrict__ top, int rows,
                                          int cols, int iterations, unsigned char* __restrict__ out, unsigned char* __restrict__ mask) {
    const int npix = rows * cols;  // rows, cols <= 16384
    const bool any = *top != 0.0;  // the 1 x 1 level: 0 = no valid depth = all-zero outputs
    const int64_t stride = (int64_t)gridDim.x * kBP * 4;
    for (int64_t q0 = ((int64_t)blockIdx.x * kBP + threadIdx.x) * 4; q0 < npix; q0 += stride) {
        const int p0 = (int)q0;
        unsigned v[4 * CH], m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int c = 0; c < CH; ++c) v[CH * j + c] = 0u;
            m[j] = 0u;
            if (any && p0 + j < npix) m[j] = warp_pixel<CH>(img, disp, rows, cols, iterations, p0 + j, v + CH * j);
        }
        if (p0 + 4 <= npix) {  // p0 % 4 == 0: CH * p0 bytes are 4-byte aligned
            unsigned* dst = reinterpret_cast<unsigned*>(out + (int64_t)CH * p0);
#pragma unroll
            for (int d = 0; d < CH; ++d) dst[d] = v[4 * d] | (v[4 * d + 1] << 8) | (v[4 * d + 2] << 16) | (v[4 * d + 3] << 24);
            if (mask) *reinterpret_cast<unsigned*>(mask + p0) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p0 + j < npix) {
#pragma unroll
                    for (int c = 0; c < CH; ++c) out[(int64_t)CH * (p0 + j) + c] = (unsigned char)v[CH * j + c];
                    if (mask) mask[p0 + j] = (unsigned char)m[j];
                }
        }
    }
}

}  // namespace

}  // namespace rsdsfm
