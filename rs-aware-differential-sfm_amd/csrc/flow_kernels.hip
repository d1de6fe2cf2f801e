// flow_kernels.hip -- the DeepFlow front end's kernels for one pair (Camera::calculateDeepFlow, camera.cc:253-277).
//
// Thin wrappers: every body lives in flow_device.hpp, which the batched sequence kernels (flow_seq_kernels.hip) share, so both paths
// give the same bits.  Every per-pixel quantity is float32 with one rounding per operation, in the order tests/flow_spec_numpy.py
// writes it.  No kernel here may need a private segment.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_device.hpp"
#include "flow_kernels.hpp"

namespace rsdsfm {
namespace {

using namespace flowdev;

// gray conversion + horizontal pass of the pre-smoothing (blockIdx.z = image)
__global__ __launch_bounds__(kLineBlock) void flow_gray_hblur_kernel(const uint8_t* __restrict__ img1, const uint8_t* __restrict__ img2, int rows,
                                                                    int cols, int channels, const float* __restrict__ taps, int radius,
                                                                    float* __restrict__ out1, float* __restrict__ out2) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    gray_hblur_px(blockIdx.z ? img2 : img1, cols, channels, taps, radius, blockIdx.z ? out2 : out1, x, y);
}

// vertical pass of the pre-smoothing
__global__ __launch_bounds__(kLineBlock) void flow_vblur_kernel(const float* __restrict__ in1, const float* __restrict__ in2, int rows, int cols,
                                                               const float* __restrict__ taps, int radius, float* __restrict__ out1,
                                                               float* __restrict__ out2) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    vblur_px(blockIdx.z ? in2 : in1, rows, cols, taps, radius, blockIdx.z ? out2 : out1, x, y);
}

// one pyramid level from the previous one (both images)
__global__ __launch_bounds__(kLineBlock) void flow_pyr_down_kernel(const float* __restrict__ src1, const float* __restrict__ src2, int scols,
                                                                  FlowResizeTab tab, int rows, int cols, float* __restrict__ dst1,
                                                                  float* __restrict__ dst2) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    pyr_down_px(blockIdx.z ? src2 : src1, scols, tab, cols, blockIdx.z ? dst2 : dst1, x, y);
}

// level entry: upsampled coarser flow, warp of image 2, zero increment, averaged image, temporal difference
__global__ __launch_bounds__(kLineBlock) void flow_entry_kernel(FlowLevelBufs L, const float* __restrict__ i1, const float* __restrict__ i2,
                                                               int rows, int cols, FlowCoarse C, float scale) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    entry_px(L, i1, i2, rows, cols, C, scale, x, y);
}

// first and second derivatives
__global__ __launch_bounds__(kLineBlock) void flow_deriv_kernel(FlowLevelBufs L, int rows, int cols) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    deriv_px(L, rows, cols, x, y);
}

// the 2x2 system of one fixed-point iteration
__global__ __launch_bounds__(kLineBlock) void flow_coef_kernel(FlowLevelBufs L, int rows, int cols, FlowConsts k) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    coef_px(L, rows, cols, k, x, y);
}

// red-black SOR, one kFlowRegion x kFlowRegion region per workgroup (blockIdx.x = region)
__global__ __launch_bounds__(kFlowSorThreads) void flow_sor_kernel(FlowSorArgs a) { sor_region(a, blockIdx.x); }

// level 0: flow = (u + du, v + dv) widened to f64, interleaved
__global__ __launch_bounds__(kLineBlock) void flow_output_kernel(FlowLevelBufs L, int rows, int cols, double* __restrict__ flow) {
    const int x = blockIdx.x * kLineBlock + threadIdx.x, y = blockIdx.y;
    if (x >= cols || y >= rows) return;
    output_px(L, cols, flow, x, y);
}

dim3 line_grid(int rows, int cols, int z) { return dim3((unsigned)((cols + kLineBlock - 1) / kLineBlock), (unsigned)rows, (unsigned)z); }

}  // namespace

hipError_t flow_presmooth(hipStream_t s, const uint8_t* img1, const uint8_t* img2, int rows, int cols, int channels, const float* taps, int radius,
                          float* tmp1, float* tmp2, float* out1, float* out2) {
    hipLaunchKernelGGL(flow_gray_hblur_kernel, line_grid(rows, cols, 2), dim3(kLineBlock), 0, s, img1, img2, rows, cols, channels, taps, radius, tmp1, tmp2);
    hipLaunchKernelGGL(flow_vblur_kernel, line_grid(rows, cols, 2), dim3(kLineBlock), 0, s, tmp1, tmp2, rows, cols, taps, radius, out1, out2);
    return hipGetLastError();
}

hipError_t flow_pyr_down(hipStream_t s, const float* src1, const float* src2, int scols, const FlowResizeTab& tab, int rows, int cols, float* dst1,
                         float* dst2) {
    hipLaunchKernelGGL(flow_pyr_down_kernel, line_grid(rows, cols, 2), dim3(kLineBlock), 0, s, src1, src2, scols, tab, rows, cols, dst1, dst2);
    return hipGetLastError();
}

hipError_t flow_level_entry(hipStream_t s, const FlowLevelBufs& L, const float* i1, const float* i2, int rows, int cols, const FlowCoarse& C,
                            float scale) {
    hipLaunchKernelGGL(flow_entry_kernel, line_grid(rows, cols, 1), dim3(kLineBlock), 0, s, L, i1, i2, rows, cols, C, scale);
    hipLaunchKernelGGL(flow_deriv_kernel, line_grid(rows, cols, 1), dim3(kLineBlock), 0, s, L, rows, cols);
    return hipGetLastError();
}

hipError_t flow_coef(hipStream_t s, const FlowLevelBufs& L, int rows, int cols, const FlowConsts& k) {
    hipLaunchKernelGGL(flow_coef_kernel, line_grid(rows, cols, 1), dim3(kLineBlock), 0, s, L, rows, cols, k);
    return hipGetLastError();
}

hipError_t flow_sor(hipStream_t s, const FlowSorArgs& a, int tiles) {
    hipLaunchKernelGGL(flow_sor_kernel, dim3((unsigned)tiles), dim3(kFlowSorThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t flow_output(hipStream_t s, const FlowLevelBufs& L, int rows, int cols, double* flow) {
    hipLaunchKernelGGL(flow_output_kernel, line_grid(rows, cols, 1), dim3(kLineBlock), 0, s, L, rows, cols, flow);
    return hipGetLastError();
}

}  // namespace rsdsfm
