// flow_device.hpp -- the per-pixel (and per-region) bodies of the DeepFlow front end's kernels, shared by the
// single-pair kernels (flow_kernels.hip) and the batched sequence kernels (flow_seq_kernels.hip): each stage has one
// implementation, so both paths compute the same expressions in the same order and give the same bits.
//
// Every per-pixel quantity is float32 with one rounding per operation, in the order tests/flow_spec_numpy.py writes it (the build
// runs with -ffp-contract=off; fp32 `/` and sqrtf are correctly rounded), so the field is the spec's bit for bit.  Gaussian taps
// and resize weights come from the host (double, rounded once).  One lane per pixel, no MFMA.  No kernel may need a private
// segment: per-pixel register arrays are indexed by compile-time constants only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_kernels.hpp"

namespace rsdsfm {
namespace flowdev {

constexpr float kZeta2 = 0.01f;
constexpr float kEps2 = 1e-6f;
constexpr int kLineBlock = 256;  // per-pixel kernels: one row segment of 256 pixels per workgroup

__device__ __forceinline__ int clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    i = abs(i) % period;
    return i >= n ? period - i : i;
}

__device__ __forceinline__ float gray_at(const uint8_t* __restrict__ img, size_t idx, int channels) {
    if (channels == 3) {
        const uint8_t* p = img + 3 * idx;
        return (float)((1868 * (int)p[0] + 9617 * (int)p[1] + 4899 * (int)p[2] + 8192) >> 14);
    }
    return (float)img[idx];
}

// gray conversion + horizontal pass of the pre-smoothing at (y, x)
__device__ __forceinline__ void gray_hblur_px(const uint8_t* __restrict__ img, int cols, int channels, const float* __restrict__ taps, int radius,
                                              float* __restrict__ out, int x, int y) {
    const size_t row = (size_t)y * cols;
    float acc = taps[0] * gray_at(img, row + reflect101(x - radius, cols), channels);
    for (int i = 1; i <= 2 * radius; ++i) acc = acc + taps[i] * gray_at(img, row + reflect101(x - radius + i, cols), channels);
    out[row + x] = acc;
}

// vertical pass of the pre-smoothing at (y, x)
__device__ __forceinline__ void vblur_px(const float* __restrict__ in, int rows, int cols, const float* __restrict__ taps, int radius,
                                         float* __restrict__ out, int x, int y) {
    float acc = taps[0] * in[(size_t)reflect101(y - radius, rows) * cols + x];
    for (int i = 1; i <= 2 * radius; ++i) acc = acc + taps[i] * in[(size_t)reflect101(y - radius + i, rows) * cols + x];
    out[(size_t)y * cols + x] = acc;
}

// bilinear resize with host tables: r0 = wx0 f[y0][x0] + wx1 f[y0][x1], r1 likewise on row y1, out = wy0 r0 + wy1 r1
__device__ __forceinline__ float resize_at(const float* __restrict__ f, int scols, const FlowResizeTab& t, int x, int y) {
    const int x0 = t.x0[x], x1 = t.x1[x], y0 = t.y0[y], y1 = t.y1[y];
    const float wx0 = t.wx0[x], wx1 = t.wx1[x];
    const float r0 = wx0 * f[(size_t)y0 * scols + x0] + wx1 * f[(size_t)y0 * scols + x1];
    const float r1 = wx0 * f[(size_t)y1 * scols + x0] + wx1 * f[(size_t)y1 * scols + x1];
    return t.wy0[y] * r0 + t.wy1[y] * r1;
}

// one pyramid level from the previous one at (y, x)
__device__ __forceinline__ void pyr_down_px(const float* __restrict__ src, int scols, const FlowResizeTab& tab, int cols, float* __restrict__ dst, int x,
                                            int y) {
    dst[(size_t)y * cols + x] = resize_at(src, scols, tab, x, y);
}

// level entry at (y, x): flow of the coarser level (u + du, resized, times 1/downscale; zero on the coarsest level), warp of image 2
// by it, the increment set to zero, the averaged image and the temporal difference
__device__ __forceinline__ void entry_px(const FlowLevelBufs& L, const float* __restrict__ i1, const float* __restrict__ i2, int rows, int cols,
                                         const FlowCoarse& C, float scale, int x, int y) {
    const size_t i = (size_t)y * cols + x;
    float u = 0.f, v = 0.f;
    if (C.u) {
        const int x0 = C.tab.x0[x], x1 = C.tab.x1[x], y0 = C.tab.y0[y], y1 = C.tab.y1[y];
        const float wx0 = C.tab.wx0[x], wx1 = C.tab.wx1[x], wy0 = C.tab.wy0[y], wy1 = C.tab.wy1[y];
        const size_t a = (size_t)y0 * C.cols + x0, b = (size_t)y0 * C.cols + x1, c = (size_t)y1 * C.cols + x0, d = (size_t)y1 * C.cols + x1;
        const float ua = C.u[a] + C.du[a], ub = C.u[b] + C.du[b], uc = C.u[c] + C.du[c], ud = C.u[d] + C.du[d];
        const float va = C.v[a] + C.dv[a], vb = C.v[b] + C.dv[b], vc = C.v[c] + C.dv[c], vd = C.v[d] + C.dv[d];
        u = (wy0 * (wx0 * ua + wx1 * ub) + wy1 * (wx0 * uc + wx1 * ud)) * scale;
        v = (wy0 * (wx0 * va + wx1 * vb) + wy1 * (wx0 * vc + wx1 * vd)) * scale;
    }
    const float X = fminf(fmaxf((float)x + u, -1.f), (float)cols);
    const float Y = fminf(fmaxf((float)y + v, -1.f), (float)rows);
    const float fx = floorf(X), fy = floorf(Y);
    const float ax = X - fx, ay = Y - fy;
    const float bx = 1.f - ax, by = 1.f - ay;
    const int xi = (int)fx, yi = (int)fy;
    const int xa = clampi(xi, 0, cols - 1), xb = clampi(xi + 1, 0, cols - 1);
    const int ya = clampi(yi, 0, rows - 1), yb = clampi(yi + 1, 0, rows - 1);
    const float r0 = bx * i2[(size_t)ya * cols + xa] + ax * i2[(size_t)ya * cols + xb];
    const float r1 = bx * i2[(size_t)yb * cols + xa] + ax * i2[(size_t)yb * cols + xb];
    const float w = by * r0 + ay * r1;
    const float g = i1[i];
    L.u[i] = u;
    L.v[i] = v;
    L.du[i] = 0.f;
    L.dv[i] = 0.f;
    L.avg[i] = 0.5f * (g + w);
    L.d[FLOW_IZ][i] = w - g;
}

// central differences (replicate border) at (y, x): first derivatives of the averaged image and of Iz, second derivatives by
// recomputing the first ones at the neighbours (the same operations as on a stored plane)
__device__ __forceinline__ void deriv_px(const FlowLevelBufs& L, int rows, int cols, int x, int y) {
    const float* __restrict__ A = L.avg;
    const float* __restrict__ Z = L.d[FLOW_IZ];
    const int xm = max(x - 1, 0), xp = min(x + 1, cols - 1), ym = max(y - 1, 0), yp = min(y + 1, rows - 1);
    auto at = [&](const float* f, int yy, int xx) { return f[(size_t)yy * cols + xx]; };
    auto ix = [&](int yy, int xx) { return 0.5f * (at(A, yy, min(xx + 1, cols - 1)) - at(A, yy, max(xx - 1, 0))); };
    auto iy = [&](int yy, int xx) { return 0.5f * (at(A, min(yy + 1, rows - 1), xx) - at(A, max(yy - 1, 0), xx)); };
    const size_t i = (size_t)y * cols + x;
    L.d[FLOW_IX][i] = ix(y, x);
    L.d[FLOW_IY][i] = iy(y, x);
    L.d[FLOW_IXX][i] = 0.5f * (ix(y, xp) - ix(y, xm));
    L.d[FLOW_IXY][i] = 0.5f * (ix(yp, x) - ix(ym, x));
    L.d[FLOW_IYY][i] = 0.5f * (iy(yp, x) - iy(ym, x));
    L.d[FLOW_IXZ][i] = 0.5f * (at(Z, y, xp) - at(Z, y, xm));
    L.d[FLOW_IYZ][i] = 0.5f * (at(Z, yp, x) - at(Z, ym, x));
}

// robust smoothness weight alpha * Psi'(|grad(u+du)|^2 + |grad(v+dv)|^2) at (y, x), forward differences (0 on the last row / column)
__device__ __forceinline__ float smooth_weight(const FlowLevelBufs L, int rows, int cols, int y, int x, float alpha) {
    const size_t i = (size_t)y * cols + x;
    const float U = L.u[i] + L.du[i], V = L.v[i] + L.dv[i];
    float ux = 0.f, uy = 0.f, vx = 0.f, vy = 0.f;
    if (x < cols - 1) {
        ux = (L.u[i + 1] + L.du[i + 1]) - U;
        vx = (L.v[i + 1] + L.dv[i + 1]) - V;
    }
    if (y < rows - 1) {
        uy = (L.u[i + cols] + L.du[i + cols]) - U;
        vy = (L.v[i + cols] + L.dv[i + cols]) - V;
    }
    const float s2 = ((ux * ux + uy * uy) + vx * vx) + vy * vy;
    return alpha * (1.f / sqrtf(s2 + kEps2));
}

// the 2x2 system of one fixed-point iteration at (y, x): A12, R1 = 1 / (A11 + sum w), R2 = 1 / (A22 + sum w), B1, B2, wL, wR, wU, wD
__device__ __forceinline__ void coef_px(const FlowLevelBufs L, int rows, int cols, const FlowConsts k, int x, int y) {
    const size_t i = (size_t)y * cols + x;
    const float Ix = L.d[FLOW_IX][i], Iy = L.d[FLOW_IY][i], Iz = L.d[FLOW_IZ][i], Ixx = L.d[FLOW_IXX][i], Ixy = L.d[FLOW_IXY][i],
                Iyy = L.d[FLOW_IYY][i], Ixz = L.d[FLOW_IXZ][i], Iyz = L.d[FLOW_IYZ][i];
    const float du = L.du[i], dv = L.dv[i];
    const float n0 = (Ix * Ix + Iy * Iy) + kZeta2;
    const float r0 = (Iz + Ix * du) + Iy * dv;
    const float p0 = 1.f / sqrtf((r0 * r0) / n0 + kEps2);
    const float k0 = (k.delta * p0) / n0;
    const float nx = (Ixx * Ixx + Ixy * Ixy) + kZeta2;
    const float ny = (Ixy * Ixy + Iyy * Iyy) + kZeta2;
    const float rx = (Ixz + Ixx * du) + Ixy * dv;
    const float ry = (Iyz + Ixy * du) + Iyy * dv;
    const float pg = 1.f / sqrtf(((rx * rx) / nx + (ry * ry) / ny) + kEps2);
    const float kx = (k.gamma * pg) / nx;
    const float ky = (k.gamma * pg) / ny;
    const float A11 = ((k0 * Ix) * Ix + (kx * Ixx) * Ixx) + (ky * Ixy) * Ixy;
    const float A12 = ((k0 * Ix) * Iy + (kx * Ixx) * Ixy) + (ky * Ixy) * Iyy;
    const float A22 = ((k0 * Iy) * Iy + (kx * Ixy) * Ixy) + (ky * Iyy) * Iyy;
    const float b1 = -(((k0 * Ix) * Iz + (kx * Ixx) * Ixz) + (ky * Ixy) * Iyz);
    const float b2 = -(((k0 * Iy) * Iz + (kx * Ixy) * Ixz) + (ky * Iyy) * Iyz);
    const float wgt = smooth_weight(L, rows, cols, y, x, k.alpha);
    const float wR = x < cols - 1 ? wgt : 0.f;
    const float wD = y < rows - 1 ? wgt : 0.f;
    const float wL = x > 0 ? smooth_weight(L, rows, cols, y, x - 1, k.alpha) : 0.f;
    const float wU = y > 0 ? smooth_weight(L, rows, cols, y - 1, x, k.alpha) : 0.f;
    const float W = ((wL + wR) + wU) + wD;
    const size_t iL = (size_t)y * cols + max(x - 1, 0), iR = (size_t)y * cols + min(x + 1, cols - 1);
    const size_t iU = (size_t)max(y - 1, 0) * cols + x, iD = (size_t)min(y + 1, rows - 1) * cols + x;
    const float u = L.u[i], v = L.v[i];
    const float pu = ((wL * (L.u[iL] - u) + wR * (L.u[iR] - u)) + wU * (L.u[iU] - u)) + wD * (L.u[iD] - u);
    const float pv = ((wL * (L.v[iL] - v) + wR * (L.v[iR] - v)) + wU * (L.v[iU] - v)) + wD * (L.v[iD] - v);
    L.c[FLOW_A12][i] = A12;
    L.c[FLOW_R1][i] = 1.f / (A11 + W);
    L.c[FLOW_R2][i] = 1.f / (A22 + W);
    L.c[FLOW_B1][i] = b1 + pu;
    L.c[FLOW_B2][i] = b2 + pv;
    L.c[FLOW_WL][i] = wL;
    L.c[FLOW_WR][i] = wR;
    L.c[FLOW_WU][i] = wU;
    L.c[FLOW_WD][i] = wD;
}

// Red-black SOR with temporal blocking, region `tile` of the level (the body of a kFlowSorThreads workgroup).  A workgroup owns a
// kFlowRegion x kFlowRegion region of the level: its interior (kFlowRegion - 2 halo per side) plus a halo; du / dv of the region
// live in LDS (one zero cell around it), the nine coefficients of its pixels in registers.  `nit` iterations (2 nit half-sweeps)
// run before the interior is written: a wrong value enters at the region's edge (the zero ring) and moves one pixel per half-sweep,
// so with halo >= 2 nit the interior is exact.  A region that reaches the image border on a side has the true zero padding there.
// Thread t owns the pixel pair (2 (t % 32), 2 (t % 32) + 1) of rows t / 32 + 32 j: one of the two has the colour of each
// half-sweep (no idle lanes).  The update is branch-free: an out-of-image pixel has all-zero coefficients, so it stays exactly +0
// (the zero padding of the spec) and contributes 0 to its neighbours.  Red-black order makes every value independent of the tiling.
// The arguments come by value: taken by reference, flow_sor_kernel needed 79 VGPRs instead of 72.
__device__ __forceinline__ void sor_region(const FlowSorArgs a, unsigned tile) {
    constexpr int R = kFlowRegion, LW = kFlowRegion + 2, PAIRS = kFlowRegion / 2, RG = kFlowSorThreads / PAIRS, NJ = kFlowRegion / RG;
    static_assert(RG * NJ == kFlowRegion && PAIRS * RG == kFlowSorThreads, "region / thread layout");
    __shared__ float sdu[(R + 2) * LW];
    __shared__ float sdv[(R + 2) * LW];
    const int tw = R - 2 * a.halo, th = R - 2 * a.halo;
    const int X0 = (int)(tile % a.tiles_x) * tw - a.halo, Y0 = (int)(tile / a.tiles_x) * th - a.halo;
    for (int i = threadIdx.x; i < (R + 2) * LW; i += kFlowSorThreads) {
        sdu[i] = 0.f;
        sdv[i] = 0.f;
    }
    __syncthreads();
    const int pr = threadIdx.x % PAIRS, rg = threadIdx.x / PAIRS;
    float cA12[NJ][2], cR1[NJ][2], cR2[NJ][2], cB1[NJ][2], cB2[NJ][2], cwL[NJ][2], cwR[NJ][2], cwU[NJ][2], cwD[NJ][2];
    bool inside[NJ][2];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int gy = Y0 + rg + RG * j;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int gx = X0 + 2 * pr + e;
            const bool ok = gy >= 0 && gy < a.rows && gx >= 0 && gx < a.cols;
            inside[j][e] = ok;
            cA12[j][e] = cR1[j][e] = cR2[j][e] = cB1[j][e] = cB2[j][e] = cwL[j][e] = cwR[j][e] = cwU[j][e] = cwD[j][e] = 0.f;
            if (ok) {
                const size_t i = (size_t)gy * a.cols + gx;
                cA12[j][e] = a.c[FLOW_A12][i];
                cR1[j][e] = a.c[FLOW_R1][i];
                cR2[j][e] = a.c[FLOW_R2][i];
                cB1[j][e] = a.c[FLOW_B1][i];
                cB2[j][e] = a.c[FLOW_B2][i];
                cwL[j][e] = a.c[FLOW_WL][i];
                cwR[j][e] = a.c[FLOW_WR][i];
                cwU[j][e] = a.c[FLOW_WU][i];
                cwD[j][e] = a.c[FLOW_WD][i];
                const int s = (rg + RG * j + 1) * LW + 2 * pr + e + 1;
                sdu[s] = a.du_in[i];
                sdv[s] = a.dv_in[i];
            }
        }
    }
    __syncthreads();
    for (int it = 0; it < a.nit; ++it) {
#pragma unroll
        for (int color = 0; color < 2; ++color) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int gy = Y0 + rg + RG * j;
                const int e = ((X0 + 2 * pr + gy) & 1) ^ color;  // red = (row + col) even
                {
                    const float A12 = e ? cA12[j][1] : cA12[j][0], R1 = e ? cR1[j][1] : cR1[j][0], R2 = e ? cR2[j][1] : cR2[j][0];
                    const float B1 = e ? cB1[j][1] : cB1[j][0], B2 = e ? cB2[j][1] : cB2[j][0];
                    const float wL = e ? cwL[j][1] : cwL[j][0], wR = e ? cwR[j][1] : cwR[j][0];
                    const float wU = e ? cwU[j][1] : cwU[j][0], wD = e ? cwD[j][1] : cwD[j][0];
                    const int s = (rg + RG * j + 1) * LW + 2 * pr + e + 1;
                    const float du = sdu[s], dv = sdv[s];
                    const float su = ((wL * sdu[s - 1] + wR * sdu[s + 1]) + wU * sdu[s - LW]) + wD * sdu[s + LW];
                    const float dun = a.om1 * du + a.om * (((B1 + su) - A12 * dv) * R1);
                    const float sv = ((wL * sdv[s - 1] + wR * sdv[s + 1]) + wU * sdv[s - LW]) + wD * sdv[s + LW];
                    const float dvn = a.om1 * dv + a.om * (((B2 + sv) - A12 * dun) * R2);
                    sdu[s] = dun;
                    sdv[s] = dvn;
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int ry = rg + RG * j;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int rx = 2 * pr + e;
            if (inside[j][e] && rx >= a.halo && rx < a.halo + tw && ry >= a.halo && ry < a.halo + th) {
                const size_t i = (size_t)(Y0 + ry) * a.cols + (X0 + rx);
                const int s = (ry + 1) * LW + rx + 1;
                a.du_out[i] = sdu[s];
                a.dv_out[i] = sdv[s];
            }
        }
    }
}

// level 0 at (y, x): flow = (u + du, v + dv) widened to f64, interleaved
__device__ __forceinline__ void output_px(const FlowLevelBufs& L, int cols, double* __restrict__ flow, int x, int y) {
    const size_t i = (size_t)y * cols + x;
    flow[2 * i] = (double)(L.u[i] + L.du[i]);
    flow[2 * i + 1] = (double)(L.v[i] + L.dv[i]);
}

}  // namespace flowdev
}  // namespace rsdsfm
