// stabilize_search_kernels.hip -- the stabiliser's search for the visible pre-image on MI355X (gfx950): include/rsdsfm_stabilize_search.h,
// defined by tests/stabilize_search_spec_numpy.py and reproduced bit for bit (float64 arithmetic, one rounding per operation,
// -ffp-contract=off).  Stage A (the inverse-depth fill) is the dense rectifier's launch, unchanged; this file has
//   B++  stabilize_search_map_kernel   stabilize_map_kernel's statements (stabilize_map_body.hpp) with the zv store of the occlusion test's
//                                      map kernel and the splat as a 64-bit KEY, bits(zv) << 32 | source index: a plain load of the cell
//                                      first, then an integer atomic minimum without a returned value only when the cell holds more than the
//                                      lane's key.  8 B read, 12 B written per pixel and at most one 8-byte atomic.
//   C++  stabilize_search_warp_kernel / stabilize_search_warp_gray_kernel (3 / 1 channels)
//                                      window_warp_body's structure (stabilize_crop_kernels.hip) -- 4 pixels per thread, the mask's dword
//                                      first, done at 1 B per pixel where it is 0x01010101, merged write-back, byte tail -- with, for a pixel
//                                      that is still empty and valid, ONE 3 x 3 read of the keys (72 B) that serves both the test's zn (the
//                                      high word of the minimum) and the restart (its low word), the 4 loads of zv of the test and, only for
//                                      lanes that failed it, the restart: the fixed point again from the source pixel the key names, 4 more
//                                      loads of zv and the sample.  Taken, rejected and recovered pixels are summed through wave shuffles
//                                      and LDS to one 64-bit integer atomicAdd each per workgroup.
#include <algorithm>

#include "rectify_dense.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_search.hpp"
#include "stabilize_window_device.hpp"

namespace rsdsfm {

namespace {

// warp_fixed_point (stabilize_window_device.hpp) started at (px, py) instead of at the target: p <- t - D(p); returns the validity of p
__device__ __forceinline__ bool search_fixed_point(const float2* __restrict__ disp, int rows, int cols, int iterations, double gx, double gy, double& px, double& py) {
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

// the occlusion test's decision at the taps (ax, ay) against zn (zlim = (double)zn k; zn all ones: no evidence, visible)
__device__ __forceinline__ bool search_visible(const float* __restrict__ zv, int cols, const Tap& ax, const Tap& ay, unsigned zn, double zlim) {
    const float* z0 = zv + (int64_t)ay.i0 * cols;
    const float* z1 = zv + (int64_t)ay.i1 * cols;
    const float z00 = z0[ax.i0], z01 = z0[ax.i1], z10 = z1[ax.i0], z11 = z1[ax.i1];
    if (z00 == 0.0f || z01 == 0.0f || z10 == 0.0f || z11 == 0.0f) return false;
    const double zs = lerp(lerp((double)z00, (double)z01, ax.a), lerp((double)z10, (double)z11, ax.a), ay.a);
    return zn == kKeyHighEmpty || !(zs > zlim);
}

// one output pixel: 0 = stage C's fixed point is not valid, 1 = taken, 2 = rejected, 3 = recovered (bit 0: v[CH] is the pixel; else v is 0)
template <int CH>
__device__ __forceinline__ unsigned search_pixel(const unsigned char* __restrict__ img, const float2* __restrict__ disp, const float* __restrict__ zv,
                                                 const unsigned long long* __restrict__ kbuf, int rows, int cols, int iterations, const CropMap& wm, double k, int p,
                                                 unsigned* v) {
#pragma unroll
    for (int c = 0; c < CH; ++c) v[c] = 0u;
    double tx, ty, px, py;
    window_target(wm, cols, p, tx, ty);
    if (!warp_fixed_point(disp, rows, cols, iterations, tx, ty, px, py)) return 0u;
    const int jc = (int)fmin(fmax(tx + 0.5, 0.0), (double)(cols - 1)), ic = (int)fmin(fmax(ty + 0.5, 0.0), (double)(rows - 1));  // inside the plane
    unsigned long long kn = kKeyEmpty;
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj) {
            const int i = ic + di, j = jc + dj;
            if (i >= 0 && i < rows && j >= 0 && j < cols) kn = min(kn, kbuf[(int64_t)i * cols + j]);
        }
    const unsigned zn = (unsigned)(kn >> 32);
    const double zlim = (double)__uint_as_float(zn) * k;  // (not read where zn is empty)
    const Tap ax = tap(px, cols), ay = tap(py, rows);     // the taps of the image sample
    if (search_visible(zv, cols, ax, ay, zn, zlim)) {
        warp_sample<CH>(img, cols, ax, ay, true, v);
        return 1u;
    }
    if (kn == kKeyEmpty) return 2u;  // nothing landed there: nowhere to start from
    const int src = (int)(unsigned)kn, sy = src / cols, sx = src - sy * cols;  // the source pixel nearest the camera on that cell: < rows cols
    double qx = (double)sx, qy = (double)sy;
    if (!search_fixed_point(disp, rows, cols, iterations, tx, ty, qx, qy)) return 2u;
    const Tap bx = tap(qx, cols), by = tap(qy, rows);
    if (!search_visible(zv, cols, bx, by, zn, zlim)) return 2u;
    warp_sample<CH>(img, cols, bx, by, true, v);
    return 3u;
}

template <int CH>
__device__ __forceinline__ void search_warp_body(const unsigned char* __restrict__ img, const float2* __restrict__ disp, const float* __restrict__ zv,
                                                 const unsigned long long* __restrict__ kbuf, const double* __restrict__ top, int rows, int cols, int iterations,
                                                 unsigned sid, const CropMap wm, double k, unsigned char* __restrict__ out, unsigned char* __restrict__ mask,
                                                 unsigned char* __restrict__ source, unsigned long long* __restrict__ counts3) {
    __shared__ unsigned s_wave[3][kBP / 64];
    const int npix = rows * cols;    // rows, cols <= 16384
    unsigned n = 0, nr = 0, ns = 0;  // taken, rejected, recovered: at most 4 per step and 2^28 / 4 steps in all: no overflow
    if (*top != 0.0) {               // the 1 x 1 level: 0 = the frame has no valid depth = it offers nothing (uniform)
        const int64_t stride = (int64_t)gridDim.x * kBP * 4;
        for (int64_t q0 = ((int64_t)blockIdx.x * kBP + threadIdx.x) * 4; q0 < npix; q0 += stride) {
            const int p0 = (int)q0;
            if (p0 + 4 <= npix) {  // p0 % 4 == 0: p0 and CH * p0 bytes are 4-byte aligned
                unsigned* mw = reinterpret_cast<unsigned*>(mask + p0);
                const unsigned old = *mw;
                if (old == 0x01010101u) continue;
                unsigned v[4 * CH], t[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int c = 0; c < CH; ++c) v[CH * j + c] = 0u;
                    t[j] = 0u;
                    if (((old >> (8 * j)) & 0xffu) == 0u) {
                        const unsigned r = search_pixel<CH>(img, disp, zv, kbuf, rows, cols, iterations, wm, k, p0 + j, v + CH * j);
                        t[j] = r & 1u;
                        n += r == 1u ? 1u : 0u;
                        nr += r == 2u ? 1u : 0u;
                        ns += r == 3u ? 1u : 0u;
                    }
                }
                const unsigned take = t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24);  // 1 in the bytes of the pixels taken or recovered
                if (take == 0u) continue;
                unsigned* dst = reinterpret_cast<unsigned*>(out + (int64_t)CH * p0);
                if (take == 0x01010101u) {  // nothing of the 4 pixels is kept: no read
#pragma unroll
                    for (int d = 0; d < CH; ++d) dst[d] = v[4 * d] | (v[4 * d + 1] << 8) | (v[4 * d + 2] << 16) | (v[4 * d + 3] << 24);
                    if (source) *reinterpret_cast<unsigned*>(source + p0) = sid * 0x01010101u;
                } else {  // (v is 0 in the bytes of the pixels not written)
#pragma unroll
                    for (int d = 0; d < CH; ++d) {
                        const unsigned sel = (t[4 * d / CH] | (t[(4 * d + 1) / CH] << 8) | (t[(4 * d + 2) / CH] << 16) | (t[(4 * d + 3) / CH] << 24)) * 0xffu;
                        dst[d] = (dst[d] & ~sel) | (v[4 * d] | (v[4 * d + 1] << 8) | (v[4 * d + 2] << 16) | (v[4 * d + 3] << 24));
                    }
                    if (source) {
                        unsigned* sw = reinterpret_cast<unsigned*>(source + p0);
                        *sw = (*sw & ~(take * 0xffu)) | (take * sid);  // sid <= 255: no carry between the bytes
                    }
                }
                *mw = old | take;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (p0 + j < npix && mask[p0 + j] == 0) {
                        unsigned v[CH];
                        const unsigned r = search_pixel<CH>(img, disp, zv, kbuf, rows, cols, iterations, wm, k, p0 + j, v);
                        n += r == 1u ? 1u : 0u;
                        nr += r == 2u ? 1u : 0u;
                        ns += r == 3u ? 1u : 0u;
                        if (r & 1u) {
#pragma unroll
                            for (int c = 0; c < CH; ++c) out[(int64_t)CH * (p0 + j) + c] = (unsigned char)v[c];
                            mask[p0 + j] = 1;
                            if (source) source[p0 + j] = (unsigned char)sid;
                        }
                    }
            }
        }
    }
    if (!counts3) return;  // (uniform)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n += __shfl_down(n, off, 64);
        nr += __shfl_down(nr, off, 64);
        ns += __shfl_down(ns, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_wave[0][threadIdx.x / 64] = n;
        s_wave[1][threadIdx.x / 64] = nr;
        s_wave[2][threadIdx.x / 64] = ns;
    }
    __syncthreads();
    if (threadIdx.x < 3) {  // thread 0: taken, thread 1: rejected, thread 2: recovered
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kBP / 64; ++w) total += s_wave[threadIdx.x][w];
        if (total) atomicAdd(counts3 + threadIdx.x, (unsigned long long)total);
    }
}

}  // namespace

// grid: (ceil(cols / kTX), ceil(rows / kTY)), block kCB: stabilize_map_kernel with zv (rows x cols floats) and kbuf (rows x cols uint64, reset
// to all ones before the launch).  The statements are stabilize_map_body.hpp's, shared as text (see there for why)
__global__ __launch_bounds__(kCB) void stabilize_search_map_kernel(const double* __restrict__ depth_cm, const double* __restrict__ lv1, int h1, int w1,
                                                                  const double* __restrict__ R, const double* __restrict__ t, double fx, double fy, double cx,
                                                                  double cy, double fyp, int rows, int cols, int mode, StabPose vp, float2* __restrict__ disp,
                                                                  double* __restrict__ filled_cm, float* __restrict__ zv, unsigned long long* kbuf) {
#define RSDSFM_STABILIZE_MAP_VISIBLE 2
#include "stabilize_map_body.hpp"
#undef RSDSFM_STABILIZE_MAP_VISIBLE
}

// grid-stride over groups of 4 pixels, block kBP: as stabilize_visible_warp_kernel.  r0 / c0 / sy / sx: the window (CropMap); k = 1 + tol
__global__ __launch_bounds__(kBP) void stabilize_search_warp_kernel(const unsigned char* __restrict__ img, const float2* __restrict__ disp,
                                                                   const float* __restrict__ zv, const unsigned long long* __restrict__ kbuf,
                                                                   const double* __restrict__ top, int rows, int cols, int iterations, unsigned sid, double r0,
                                                                   double c0, double sy, double sx, double k, unsigned char* __restrict__ out,
                                                                   unsigned char* __restrict__ mask, unsigned char* __restrict__ source,
                                                                   unsigned long long* __restrict__ counts3) {
    search_warp_body<3>(img, disp, zv, kbuf, top, rows, cols, iterations, sid, CropMap{r0, c0, sy, sx}, k, out, mask, source, counts3);
}

__global__ __launch_bounds__(kBP) void stabilize_search_warp_gray_kernel(const unsigned char* __restrict__ img, const float2* __restrict__ disp,
                                                                        const float* __restrict__ zv, const unsigned long long* __restrict__ kbuf,
                                                                        const double* __restrict__ top, int rows, int cols, int iterations, unsigned sid,
                                                                        double r0, double c0, double sy, double sx, double k, unsigned char* __restrict__ out,
                                                                        unsigned char* __restrict__ mask, unsigned char* __restrict__ source,
                                                                        unsigned long long* __restrict__ counts3) {
    search_warp_body<1>(img, disp, zv, kbuf, top, rows, cols, iterations, sid, CropMap{r0, c0, sy, sx}, k, out, mask, source, counts3);
}

// ---------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------
int stabilize_search_launch(Ctx* c, const DenseWs& ws, const SearchWs& sw, const unsigned char* d_img_n, int channels, const double* d_depth_cm, const double* d_R,
                            const double* d_t, double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp,
                            int source_id, const int32_t window[4], unsigned char* d_out, unsigned char* d_mask, unsigned char* d_source, int tol_q16,
                            int64_t* d_counts3) {
    const double* top = nullptr;
    const int rc = rectify_dense_launch_fill(c, ws, d_depth_cm, rows, cols, &top);
    if (rc != RSDSFM_OK) return rc;
    const int64_t npix = (int64_t)rows * cols;
    RSDSFM_HIP_CHECK(c, hipMemsetAsync(sw.d_kbuf, 0xff, sizeof(unsigned long long) * (size_t)npix, c->stream));
    const DensePlan p = rectify_dense_plan(rows, cols);
    const dim3 tiles((cols + kTX - 1) / kTX, (rows + kTY - 1) / kTY);
    hipLaunchKernelGGL(stabilize_search_map_kernel, tiles, dim3(kCB), 0, c->stream, d_depth_cm, ws.d_pyr, p.h[0], p.w[0], d_R, d_t, fx, fy, cx, cy,
                       q5_mode == 0 ? fx : fy, rows, cols, mode, vp, ws.d_disp, (double*)nullptr, sw.d_zv, sw.d_kbuf);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    if (d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    const int64_t nb = (npix + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    const double sy = (double)window[2] / (double)rows, sx = (double)window[3] / (double)cols;
    const double k = 1.0 + (double)tol_q16 / 65536.0;
    hipLaunchKernelGGL(channels == 3 ? stabilize_search_warp_kernel : stabilize_search_warp_gray_kernel, dim3((unsigned)std::min<int64_t>(nb, 65536)), dim3(kBP), 0,
                       c->stream, d_img_n, ws.d_disp, sw.d_zv, sw.d_kbuf, top, rows, cols, iterations, (unsigned)source_id, (double)window[0], (double)window[1], sy, sx,
                       k, d_out, d_mask, d_source, reinterpret_cast<unsigned long long*>(d_counts3));
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
