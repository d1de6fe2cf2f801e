// flow_seq_kernels.hip -- the DeepFlow front end's kernels for a batch of consecutive frame pairs ("Sequences").
//
// The same eight stages as flow_kernels.hip, with the same bodies (flow_device.hpp), so every pair's field is bit for bit the one
// rsdsfm_deep_flow_dev computes for it.  A grid dimension selects the frame (gray + horizontal blur, vertical blur, pyramid down:
// blockIdx.z) or the pair (entry, derivatives, coefficients, output: blockIdx.z; SOR: blockIdx.y).  Per-frame planes lie at
// base + frame * frame stride, per-pair planes at base + pair * pair stride; pair p reads the pyramids of frames p and p + 1 of the
// batch.  All pairs of a batch share one level geometry, one set of resize tables and one SOR tiling.  No kernel here may need a
// private segment, and the batched SOR needs no more registers or LDS than flow_sor_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_device.hpp"
#include "flow_kernels.hpp"

namespace rsdsfm {
namespace {

using namespace flowdev;

// the working planes of one pair (every plane of the batch has the same pair stride)
__device__ __forceinline__ FlowLevelBufs pair_bufs(FlowLevelBufs L, size_t off) {
    L.u += off, L.v += off, L.du += off, L.dv += off, L.avg += off;
#pragma unroll
    for (int q = 0; q < FLOW_NDERIV; ++q) L.d[q] += off;
#pragma unroll
    for (int q = 0; q < FLOW_NCOEF; ++q) L.c[q] += off;
    return L;
}

// gray conversion + horizontal pass of the pre-smoothing (blockIdx.z = frame; its output at tmp + frame * stride)
__global__ __launch_bounds__(kLineBlock) void flow_seq_gray_hblur_kernel(FlowFramePtrs img, int rows, int cols, int channels, const float* __restrict__ taps,
                                                                        int radius, float* __restrict__ tmp, size_t stride) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    gray_hblur_px(img.p[blockIdx.z], cols, channels, taps, radius, tmp + blockIdx.z * stride, x, y);
}

// vertical pass of the pre-smoothing: tmp + frame * stride -> level 0 of the frame's pyramid (pyr + frame * pstride)
__global__ __launch_bounds__(kLineBlock) void flow_seq_vblur_kernel(const float* __restrict__ tmp, size_t stride, int rows, int cols,
                                                                   const float* __restrict__ taps, int radius, float* __restrict__ pyr, size_t pstride) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    vblur_px(tmp + blockIdx.z * stride, rows, cols, taps, radius, pyr + blockIdx.z * pstride, x, y);
}

// one pyramid level from the previous one, every frame of the batch
__global__ __launch_bounds__(kLineBlock) void flow_seq_pyr_down_kernel(const float* __restrict__ src, int scols, FlowResizeTab tab, int rows, int cols,
                                                                      float* __restrict__ dst, size_t pstride) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    pyr_down_px(src + blockIdx.z * pstride, scols, tab, cols, dst + blockIdx.z * pstride, x, y);
}

// level entry of pair blockIdx.z: image 1 = this level of frame p's pyramid, image 2 = that of frame p + 1
__global__ __launch_bounds__(kLineBlock) void flow_seq_entry_kernel(FlowLevelBufs L, size_t stride, const float* __restrict__ pyr_l, size_t pstride,
                                                                   int rows, int cols, FlowCoarse C, float scale) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    const size_t off = blockIdx.z * stride;
    if (C.u) C.u += off, C.v += off, C.du += off, C.dv += off;  // (u == nullptr marks the coarsest level and stays so)
    entry_px(pair_bufs(L, off), pyr_l + blockIdx.z * pstride, pyr_l + (blockIdx.z + 1) * pstride, rows, cols, C, scale, x, y);
}

__global__ __launch_bounds__(kLineBlock) void flow_seq_deriv_kernel(FlowLevelBufs L, size_t stride, int rows, int cols) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    deriv_px(pair_bufs(L, blockIdx.z * stride), rows, cols, x, y);
}

__global__ __launch_bounds__(kLineBlock) void flow_seq_coef_kernel(FlowLevelBufs L, size_t stride, int rows, int cols, FlowConsts k) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    coef_px(pair_bufs(L, blockIdx.z * stride), rows, cols, k, x, y);
}

// red-black SOR: blockIdx.x = region of the (shared) tiling, blockIdx.y = pair
__global__ __launch_bounds__(kFlowSorThreads) void flow_seq_sor_kernel(FlowSorArgs a, size_t stride) {
    const size_t off = blockIdx.y * stride;
#pragma unroll
    for (int q = 0; q < FLOW_NCOEF; ++q) a.c[q] += off;
    a.du_in += off, a.dv_in += off, a.du_out += off, a.dv_out += off;
    sor_region(a, blockIdx.x);
}

// level 0 of pair blockIdx.z -> that pair's own f64 field
__global__ __launch_bounds__(kLineBlock) void flow_seq_output_kernel(FlowLevelBufs L, size_t stride, int rows, int cols, FlowOutPtrs out) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    output_px(pair_bufs(L, blockIdx.z * stride), cols, out.p[blockIdx.z], x, y);
}

dim3 line_grid(int rows, int cols, int z) { return dim3((unsigned)((cols + kLineBlock - 1) / kLineBlock), (unsigned)rows, (unsigned)z); }

}  // namespace

hipError_t flow_seq_presmooth(hipStream_t s, const FlowFramePtrs& img, int nframes, int rows, int cols, int channels, const float* taps, int radius,
                              float* tmp, size_t stride, float* pyr, size_t pstride) {
    hipLaunchKernelGGL(flow_seq_gray_hblur_kernel, line_grid(rows, cols, nframes), dim3(kLineBlock), 0, s, img, rows, cols, channels, taps, radius, tmp, stride);
    hipLaunchKernelGGL(flow_seq_vblur_kernel, line_grid(rows, cols, nframes), dim3(kLineBlock), 0, s, (const float*)tmp, stride, rows, cols, taps, radius, pyr,
                       pstride);
    return hipGetLastError();
}

hipError_t flow_seq_pyr_down(hipStream_t s, const float* src, int scols, const FlowResizeTab& tab, int rows, int cols, float* dst, size_t pstride,
                             int nframes) {
    hipLaunchKernelGGL(flow_seq_pyr_down_kernel, line_grid(rows, cols, nframes), dim3(kLineBlock), 0, s, src, scols, tab, rows, cols, dst, pstride);
    return hipGetLastError();
}

hipError_t flow_seq_level_entry(hipStream_t s, const FlowLevelBufs& L, size_t stride, const float* pyr_l, size_t pstride, int rows, int cols,
                                const FlowCoarse& C, float scale, int npairs) {
    hipLaunchKernelGGL(flow_seq_entry_kernel, line_grid(rows, cols, npairs), dim3(kLineBlock), 0, s, L, stride, pyr_l, pstride, rows, cols, C, scale);
    hipLaunchKernelGGL(flow_seq_deriv_kernel, line_grid(rows, cols, npairs), dim3(kLineBlock), 0, s, L, stride, rows, cols);
    return hipGetLastError();
}

hipError_t flow_seq_coef(hipStream_t s, const FlowLevelBufs& L, size_t stride, int rows, int cols, const FlowConsts& k, int npairs) {
    hipLaunchKernelGGL(flow_seq_coef_kernel, line_grid(rows, cols, npairs), dim3(kLineBlock), 0, s, L, stride, rows, cols, k);
    return hipGetLastError();
}

hipError_t flow_seq_sor(hipStream_t s, const FlowSorArgs& a, size_t stride, int tiles, int npairs) {
    hipLaunchKernelGGL(flow_seq_sor_kernel, dim3((unsigned)tiles, (unsigned)npairs), dim3(kFlowSorThreads), 0, s, a, stride);
    return hipGetLastError();
}

hipError_t flow_seq_output(hipStream_t s, const FlowLevelBufs& L, size_t stride, int rows, int cols, const FlowOutPtrs& out, int npairs) {
    hipLaunchKernelGGL(flow_seq_output_kernel, line_grid(rows, cols, npairs), dim3(kLineBlock), 0, s, L, stride, rows, cols, out);
    return hipGetLastError();
}

}  // namespace rsdsfm
