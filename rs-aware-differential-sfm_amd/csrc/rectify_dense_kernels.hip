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
#include "rsdsfm_internal.hpp"

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
__device__ __forceinline__ void rs_to_gs_chain(int x, int y, double z, const double* Rr, const double* tr, const double* R0, const double* t0, double fx, double fy,
                                               double cx, double cy, double fyp, double& gx, double& gy) {
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
    double pg[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) pg[i] = ((R0[i * 3] * pw[0] + R0[i * 3 + 1] * pw[1]) + R0[i * 3 + 2] * pw[2]) + t0[i] * 1.0;
    gx = pg[0] / pg[2] * fx + cx;
    gy = pg[1] / pg[2] * fyp + cy;
}

}  // namespace

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

int rectify_dense_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img, int channels, const double* d_depth_cm, const double* d_R, const double* d_t,
                         double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, unsigned char* d_out,
                         unsigned char* d_mask, double* d_filled_cm) {
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
    hipLaunchKernelGGL(rectify_dense_map_kernel, tiles, dim3(kCB), 0, c->stream, d_depth_cm, pyr, p.h[0], p.w[0], d_R, d_t, fx, fy, cx, cy, q5_mode == 0 ? fx : fy,
                       rows, cols, mode, ws.d_disp, d_filled_cm);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    const int64_t npix = (int64_t)rows * cols;
    const int64_t nb = (npix + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    hipLaunchKernelGGL(channels == 3 ? rectify_dense_warp_kernel : rectify_dense_warp_gray_kernel, dim3((unsigned)std::min<int64_t>(nb, 65536)), dim3(kBP), 0, c->stream,
                       d_img, ws.d_disp, top, rows, cols, iterations, d_out, d_mask);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
