// stabilize_kernels.hip -- the stabiliser's frame on MI355X (gfx950): include/rsdsfm_stabilize.h, defined by tests/stabilize_spec_numpy.py
// and reproduced bit for bit (float64 arithmetic, one rounding per operation, -ffp-contract=off).  Stage A (the inverse-depth fill) and
// stage C (the fixed-point warp) are the dense rectifier's launches, unchanged (rectify_dense_kernels.hip); this file has
//   B  stabilize_map_kernel    rectify_dense_map_kernel's structure -- a 64 x 16 tile of the column-major depth map staged through LDS, the
//                              last push step fused, a wave per scanline segment with the scanline's pose on the scalar path, the optional
//                              filled-depth write-back -- with ONE more rigid transform behind the chain's pg (the point in the first
//                              scanline's coordinates): pv = M pg + m, the virtual camera's, and the projection of pv.  M and m are kernel
//                              arguments (12 uniform doubles); the same 8 B read and 8 B written per pixel as the dense map pass.
//      stabilize_count_kernel  the number of mask pixels that are 1: the mask as 32-bit words with a byte tail, a sum per workgroup, one
//                              64-bit integer atomicAdd per workgroup -- exact and independent of scheduling.  1 B read per pixel.
#include <algorithm>

#include "rectify_dense.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize.hpp"

namespace rsdsfm {

namespace {
constexpr int kCountBlock = 256;
constexpr int kCountMaxBlocks = 1024;
}  // namespace

// grid: (ceil(cols / kTX), ceil(rows / kTY)), block kCB: as rectify_dense_map_kernel
__global__ __launch_bounds__(kCB) void stabilize_map_kernel(const double* __restrict__ depth_cm, const double* __restrict__ lv1, int h1, int w1,
                                                           const double* __restrict__ R, const double* __restrict__ t, double fx, double fy, double cx,
                                                           double cy, double fyp, int rows, int cols, int mode, StabPose vp, float2* __restrict__ disp,
                                                           double* __restrict__ filled_cm) {
#define RSDSFM_STABILIZE_MAP_VISIBLE 0
#include "stabilize_map_body.hpp"  // the kernel's statements, shared as text with stabilize_visible_map_kernel (see there for why)
#undef RSDSFM_STABILIZE_MAP_VISIBLE
}

// mask: npix bytes of 1 / 0, 4-byte aligned; *count += their sum.  grid-stride over the npix / 4 words, the npix % 4 tail bytes by one thread.
__global__ __launch_bounds__(kCountBlock) void stabilize_count_kernel(const unsigned char* __restrict__ mask, int64_t npix, unsigned long long* __restrict__ count) {
    __shared__ unsigned s_wave[kCountBlock / 64];
    const unsigned* words = reinterpret_cast<const unsigned*>(mask);
    const int64_t nwords = npix / 4;
    unsigned n = 0;  // at most 4 per word and 2^28 / 4 words in all: no overflow
    for (int64_t i = (int64_t)blockIdx.x * kCountBlock + threadIdx.x; i < nwords; i += (int64_t)gridDim.x * kCountBlock) n += __popc(words[i] & 0x01010101u);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = nwords * 4; i < npix; ++i) n += mask[i] & 1u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x / 64] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kCountBlock / 64; ++w) total += s_wave[w];
        if (total) atomicAdd(count, (unsigned long long)total);
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int stabilize_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img, int channels, const double* d_depth_cm, const double* d_R, const double* d_t, double fx,
                     double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp, unsigned char* d_out,
                     unsigned char* d_mask, double* d_filled_cm, int64_t* d_valid) {
    const double* top = nullptr;
    int rc = rectify_dense_launch_fill(c, ws, d_depth_cm, rows, cols, &top);
    if (rc != RSDSFM_OK) return rc;
    const DensePlan p = rectify_dense_plan(rows, cols);
    const dim3 tiles((cols + kTX - 1) / kTX, (rows + kTY - 1) / kTY);
    hipLaunchKernelGGL(stabilize_map_kernel, tiles, dim3(kCB), 0, c->stream, d_depth_cm, ws.d_pyr, p.h[0], p.w[0], d_R, d_t, fx, fy, cx, cy, q5_mode == 0 ? fx : fy, rows,
                       cols, mode, vp, ws.d_disp, d_filled_cm);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    rc = rectify_dense_launch_warp(c, ws, d_img, channels, top, rows, cols, iterations, d_out, d_mask);
    if (rc != RSDSFM_OK) return rc;
    if (d_valid) {  // (d_mask is set: the caller's or the workspace's)
        const int64_t npix = (int64_t)rows * cols;
        const int64_t nb = (npix / 4 + kCountBlock - 1) / kCountBlock;
        RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_valid, 0, sizeof(int64_t), c->stream));
        hipLaunchKernelGGL(stabilize_count_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(nb, kCountMaxBlocks))), dim3(kCountBlock), 0, c->stream, d_mask,
                           npix, reinterpret_cast<unsigned long long*>(d_valid));
        RSDSFM_HIP_CHECK(c, hipGetLastError());
    }
    return RSDSFM_OK;
}

}  // namespace rsdsfm
