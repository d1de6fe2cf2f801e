// rectify_dense_kernels.hip -- the dense global-shutter frame on MI355X (gfx950): include/rsdsfm_rectify_dense.h, defined by
// tests/rectify_dense_spec_numpy.py and reproduced bit for bit (float64 arithmetic, one rounding per operation, -ffp-contract=off;
// lerp(a, b, t) = a + t * (b - a) everywhere).  One lane per pixel or cell, no MFMA, no private segment.
//
//   A  inverse-depth fill, a pull-push pyramid.  Level 0 is the column-major depth map itself and is never stored as a plane:
//      rectify_dense_pull0_kernel     stages a 64 x 16 tile of the map through LDS (coalesced along y, as the splat's claim kernel), turns it
//                                     into rho = 1 / z (0 = invalid) and writes the tile's 32 x 8 cells of LEVEL 1, row-major;
//      rectify_dense_pull_kernel      level l -> l + 1 while the levels are large;
//      rectify_dense_small_kernel     ONE workgroup: every level from the first one that (with all above it) fits 64 KB of LDS up to 1 x 1, the
//                                     whole pull and the whole push of those levels; it writes its lowest level, complete, and the 1 x 1 value;
//      rectify_dense_push_kernel      fills the zeros of level l from the complete level l + 1, down to level 1.
//   B  rectify_dense_map_kernel       the last push step and the forward map in one pass over the depth map: the tile staging above, then a
//                                     wave walks one scanline segment (pose through the scalar path), a pixel without a valid depth takes
//                                     1 / bilinear(level 1), every pixel runs the splat's chain (back_project_claim_body) and writes
//                                     D = (gx - x, gy - y) as float2; optionally the filled depth goes back through LDS, column-major.
//   C  rectify_dense_warp_kernel / _gray_kernel
//                                     p <- g - D(p) `iterations` times (four float2 gathers of a plane that sits in L2 / Infinity Cache), then the
//                                     bilinear sample of the frame; four output pixels per lane stored as packed words, bytes at the tail.
//                                     The 1 x 1 level is read here: 0 = no valid pixel = all-zero image and mask, without a host wait.
//
// Algorithmic HBM traffic per pixel (BGR): 8 B + 8 B depth read (A, B), 2.7 B pyramid written, 8 B D written, 3 B frame read, 3 B + 1 B
// written = 34 B (+ 8 B for the optional filled depth); the pyramid and D are read back through the caches.
#include <math.h>

#include <algorithm>

#include "rectify_dense.hpp"
#include "rectify_dense_device.hpp"  // the device helpers: shared with stabilize_kernels.hip
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

// grid: (ceil(cols / kTX), ceil(rows / kTY)).  Tiles start at even coordinates, so a tile holds all four children of its level-1 cells.
__global__ __launch_bounds__(kCB) void rectify_dense_pull0_kernel(const double* __restrict__ depth_cm, int rows, int cols, double* __restrict__ lv1, int h1,
                                                                 int w1) {
    __shared__ double s_r[kTX][kTY + 1];
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;
    const int tid = threadIdx.x;
    {
        const int ly = tid & (kTY - 1);
#pragma unroll
        for (int j = 0; j < kTX * kTY / kCB; ++j) {
            const int lx = tid / kTY + j * (kCB / kTY);
            const int xx = x0 + lx, yy = y0 + ly;
            s_r[lx][ly] = (xx < cols && yy < rows) ? inverse_depth(depth_cm[(int64_t)xx * rows + yy]) : 0.0;
        }
    }
    __syncthreads();
    if (tid < (kTX / 2) * (kTY / 2)) {
        const int lx = tid & (kTX / 2 - 1), ly = tid / (kTX / 2);
        const int X = x0 / 2 + lx, Y = y0 / 2 + ly;
        if (X < w1 && Y < h1)
            lv1[(int64_t)Y * w1 + X] = pull_cell(s_r[2 * lx][2 * ly], s_r[2 * lx + 1][2 * ly], s_r[2 * lx][2 * ly + 1], s_r[2 * lx + 1][2 * ly + 1]);
    }
}

// block (64, 4), one thread per cell of the coarser level
__global__ __launch_bounds__(kBP) void rectify_dense_pull_kernel(const double* __restrict__ src, int hs, int ws, double* __restrict__ dst, int hd, int wd) {
    const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y;
    if (X < wd && Y < hd) dst[(int64_t)Y * wd + X] = pull_from(src, hs, ws, X, Y);
}

// block (64, 4), one thread per cell of the finer level; valid cells are not touched
__global__ __launch_bounds__(kBP) void rectify_dense_push_kernel(double* __restrict__ lv, int h, int w, const double* __restrict__ coarser, int hc, int wc) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const int64_t i = (int64_t)y * w + x;
    if (lv[i] == 0.0) lv[i] = push_from(coarser, hc, wc, x, y);
}

// ONE workgroup.  Level S (hs x ws; its cells and those of every level above it: at most kSmallCells) comes from `src`: its own incomplete
// cells (reduce_first == 0; src may be dst) or the level below it (hsrc x wsrc), pulled here.  Pull up to 1 x 1 and push back down in LDS;
// dst = level S complete, *top = the 1 x 1 value (0: the map has no valid pixel).
__global__ __launch_bounds__(kSB) void rectify_dense_small_kernel(const double* src, int hsrc, int wsrc, int reduce_first, int hs, int ws, double* dst,
                                                                 double* top) {
    __shared__ double s[kSmallCells];
    __shared__ int s_h[kDenseMaxLevels], s_w[kDenseMaxLevels], s_off[kDenseMaxLevels];
    const int tid = threadIdx.x;
    const int n0 = hs * ws;
    for (int i = tid; i < n0; i += kSB) {
        const int Y = i / ws, X = i - Y * ws;
        s[i] = reduce_first ? pull_from(src, hsrc, wsrc, X, Y) : src[i];
    }
    int nl = 1, h = hs, w = ws, off = 0;
    if (tid == 0) s_h[0] = hs, s_w[0] = ws, s_off[0] = 0;
    __syncthreads();
    while (h > 1 || w > 1) {  // (uniform)
        const int hn = (h + 1) / 2, wn = (w + 1) / 2, offn = off + h * w;
        for (int i = tid; i < hn * wn; i += kSB) {
            const int Y = i / wn, X = i - Y * wn;
            s[offn + i] = pull_from(s + off, h, w, X, Y);
        }
        if (tid == 0) s_h[nl] = hn, s_w[nl] = wn, s_off[nl] = offn;
        ++nl;
        h = hn, w = wn, off = offn;
        __syncthreads();
    }
    for (int l = nl - 2; l >= 0; --l) {
        const int hl = s_h[l], wl = s_w[l], ol = s_off[l], hc = s_h[l + 1], wc = s_w[l + 1], oc = s_off[l + 1];
        for (int i = tid; i < hl * wl; i += kSB) {
            const int y = i / wl, x = i - y * wl;
            if (s[ol + i] == 0.0) s[ol + i] = push_from(s + oc, hc, wc, x, y);
        }
        __syncthreads();
    }
    for (int i = tid; i < n0; i += kSB) dst[i] = s[i];
    if (tid == 0) *top = s[off];
}

// grid: (ceil(cols / kTX), ceil(rows / kTY)).  A wave walks one scanline segment of 64 pixels at a time, so the scanline index is
// wave-uniform and its pose (12 doubles) comes through the scalar data path, as in the splat's claim kernel.
__global__ __launch_bounds__(kCB) void rectify_dense_map_kernel(const double* __restrict__ depth_cm, const double* __restrict__ lv1, int h1, int w1,
                                                               const double* __restrict__ R, const double* __restrict__ t, double fx, double fy, double cx,
                                                               double cy, double fyp, int rows, int cols, int mode, float2* __restrict__ disp,
                                                               double* __restrict__ filled_cm) {
    constexpr int RPW = kTY / (kCB / kTX);  // scanlines per wave
    __shared__ double s_z[kTX][kTY + 1];
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY;
    const int tid = threadIdx.x;
    const int lx = tid & (kTX - 1);
    const int x = x0 + lx;
    const int wv = __builtin_amdgcn_readfirstlane(tid / kTX);
    const int sy = tid & (kTY - 1);  // the staging layout: lanes along y
    double zst[kTX * kTY / kCB];
#pragma unroll
    for (int j = 0; j < kTX * kTY / kCB; ++j) {
        const int xx = x0 + tid / kTY + j * (kCB / kTY), yy = y0 + sy;
        zst[j] = (xx < cols && yy < rows) ? depth_cm[(int64_t)xx * rows + yy] : 0.0;
    }
    double R0[9], t0[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R0[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t0[i] = t[i];
#pragma unroll
    for (int j = 0; j < kTX * kTY / kCB; ++j) s_z[tid / kTY + j * (kCB / kTY)][sy] = zst[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
        const int ly = wv + j * (kCB / kTX);
        const int y = y0 + ly;  // wave-uniform
        // the scanline's pose, one scanline at a time: two of them beside the pose of scanline 0 do not fit the scalar registers
        double Rr[9], tr[3];
        const int ys = (mode == 0 && y < rows) ? y : 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) Rr[i] = R[(int64_t)ys * 9 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) tr[i] = t[(int64_t)ys * 3 + i];
        if (y < rows && x < cols) {
            double z = s_z[lx][ly];
            if (inverse_depth(z) == 0.0) {  // the last push step: level 0 from level 1
                const double rho = push_from(lv1, h1, w1, x, y);
                z = rho > 0.0 ? 1.0 / rho : 0.0;
                s_z[lx][ly] = z;  // (read and written by this thread only)
            }
            double gx, gy;
            rs_to_gs_chain(x, y, z, Rr, tr, R0, t0, fx, fy, cx, cy, fyp, gx, gy);
            disp[(int64_t)y * cols + x] = make_float2((float)(gx - (double)x), (float)(gy - (double)y));
        }
    }
    if (filled_cm) {  // (uniform)
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kTX * kTY / kCB; ++j) {
            const int sx = tid / kTY + j * (kCB / kTY);
            const int xx = x0 + sx, yy = y0 + sy;
            if (xx < cols && yy < rows) filled_cm[(int64_t)xx * rows + yy] = s_z[sx][sy];
        }
    }
}


__global__ __launch_bounds__(kBP) void rectify_dense_warp_kernel(const unsigned char* __restrict__ img, const float2* __restrict__ disp,
                                                                const double* __restrict__ top, int rows, int cols, int iterations,
                                                                unsigned char* __restrict__ out, unsigned char* __restrict__ mask) {
    warp_body<3>(img, disp, top, rows, cols, iterations, out, mask);
}

__global__ __launch_bounds__(kBP) void rectify_dense_warp_gray_kernel(const unsigned char* __restrict__ img, const float2* __restrict__ disp,
                                                                     const double* __restrict__ top, int rows, int cols, int iterations,
                                                                     unsigned char* __restrict__ out, unsigned char* __restrict__ mask) {
    warp_body<1>(img, disp, top, rows, cols, iterations, out, mask);
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
DensePlan rectify_dense_plan(int rows, int cols) {
    DensePlan p;
    int h = rows, w = cols;
    size_t off = 0;
    do {
        h = (h + 1) / 2, w = (w + 1) / 2;
        p.h[p.nl] = h, p.w[p.nl] = w, p.off[p.nl] = off;
        off += (size_t)h * w;
        ++p.nl;
    } while (h > 1 || w > 1);
    p.total = off;
    // the single-workgroup launch starts at the first level from which everything up to 1 x 1 fits its LDS
    p.small = p.nl - 1;
    while (p.small > 0 && p.total - p.off[p.small - 1] <= (size_t)kSmallCells) --p.small;
    return p;
}

// level 0 -> 1, the large pulls, the single-workgroup launch, the large pushes, map, warp
int rectify_dense_launch_count(int rows, int cols) {
    const DensePlan p = rectify_dense_plan(rows, cols);
    return p.small == 0 ? 4 : 1 + (p.small - 1) + 1 + p.small + 2;
}

// stage A: level 0 -> 1, the large pulls, the single-workgroup launch, the large pushes; *top = the 1 x 1 level
int rectify_dense_launch_fill(Ctx* c, const DenseWs& ws, const double* d_depth_cm, int rows, int cols, const double** top_out) {
    const DensePlan p = rectify_dense_plan(rows, cols);
    double* pyr = ws.d_pyr;
    const dim3 tiles((cols + kTX - 1) / kTX, (rows + kTY - 1) / kTY);
    const auto cells = [](int h, int w) { return dim3((w + 63) / 64, (h + 3) / 4); };
    hipLaunchKernelGGL(rectify_dense_pull0_kernel, tiles, dim3(kCB), 0, c->stream, d_depth_cm, rows, cols, pyr, p.h[0], p.w[0]);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    const int S = p.small;
    for (int l = 1; l < S; ++l) {  // levels below the single-workgroup launch's source
        hipLaunchKernelGGL(rectify_dense_pull_kernel, cells(p.h[l], p.w[l]), dim3(64, 4), 0, c->stream, pyr + p.off[l - 1], p.h[l - 1], p.w[l - 1], pyr + p.off[l],
                           p.h[l], p.w[l]);
        RSDSFM_HIP_CHECK(c, hipGetLastError());
    }
    double* top = pyr + p.off[p.nl - 1];
    if (S == 0)
        hipLaunchKernelGGL(rectify_dense_small_kernel, dim3(1), dim3(kSB), 0, c->stream, pyr, 0, 0, 0, p.h[0], p.w[0], pyr, top);
    else
        hipLaunchKernelGGL(rectify_dense_small_kernel, dim3(1), dim3(kSB), 0, c->stream, pyr + p.off[S - 1], p.h[S - 1], p.w[S - 1], 1, p.h[S], p.w[S],
                           pyr + p.off[S], top);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    for (int l = S - 1; l >= 0; --l) {
        hipLaunchKernelGGL(rectify_dense_push_kernel, cells(p.h[l], p.w[l]), dim3(64, 4), 0, c->stream, pyr + p.off[l], p.h[l], p.w[l], pyr + p.off[l + 1],
                           p.h[l + 1], p.w[l + 1]);
        RSDSFM_HIP_CHECK(c, hipGetLastError());
    }
    *top_out = top;
    return RSDSFM_OK;
}

// stage C: the fixed point on the workspace's displacement plane and the sample of the frame
int rectify_dense_launch_warp(Ctx* c, const DenseWs& ws, const unsigned char* d_img, int channels, const double* top, int rows, int cols, int iterations,
                              unsigned char* d_out, unsigned char* d_mask) {
    const int64_t npix = (int64_t)rows * cols;
    const int64_t nb = (npix + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    hipLaunchKernelGGL(channels == 3 ? rectify_dense_warp_kernel : rectify_dense_warp_gray_kernel, dim3((unsigned)std::min<int64_t>(nb, 65536)), dim3(kBP), 0, c->stream,
                       d_img, ws.d_disp, top, rows, cols, iterations, d_out, d_mask);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int rectify_dense_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img, int channels, const double* d_depth_cm, const double* d_R, const double* d_t,
                         double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, unsigned char* d_out,
                         unsigned char* d_mask, double* d_filled_cm) {
    const double* top = nullptr;
    const int rc = rectify_dense_launch_fill(c, ws, d_depth_cm, rows, cols, &top);
    if (rc != RSDSFM_OK) return rc;
    const DensePlan p = rectify_dense_plan(rows, cols);
    const dim3 tiles((cols + kTX - 1) / kTX, (rows + kTY - 1) / kTY);
    hipLaunchKernelGGL(rectify_dense_map_kernel, tiles, dim3(kCB), 0, c->stream, d_depth_cm, ws.d_pyr, p.h[0], p.w[0], d_R, d_t, fx, fy, cx, cy, q5_mode == 0 ? fx : fy,
                       rows, cols, mode, ws.d_disp, d_filled_cm);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return rectify_dense_launch_warp(c, ws, d_img, channels, top, rows, cols, iterations, d_out, d_mask);
}

}  // namespace rsdsfm
