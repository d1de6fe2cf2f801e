// flow_kernels.hpp -- interface between the DeepFlow front end's kernels (flow_kernels.hip) and its host driver (flow_host.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsdsfm {

// red-black SOR: a workgroup of kFlowSorThreads owns a kFlowRegion x kFlowRegion region in LDS; a level that fits in one region runs
// every SOR iteration of a fixed-point iteration in one launch, a larger one kFlowSorBlock iterations per launch on a halo of
// 2 kFlowSorBlock pixels (flow_sor_kernel)
constexpr int kFlowRegion = 64;
constexpr int kFlowSorThreads = 1024;
constexpr int kFlowSorBlock = 4;

// planes of the image derivatives and of the per-pixel system
enum { FLOW_IX, FLOW_IY, FLOW_IZ, FLOW_IXX, FLOW_IXY, FLOW_IYY, FLOW_IXZ, FLOW_IYZ, FLOW_NDERIV };
enum { FLOW_A12, FLOW_R1, FLOW_R2, FLOW_B1, FLOW_B2, FLOW_WL, FLOW_WR, FLOW_WU, FLOW_WD, FLOW_NCOEF };

// bilinear resize tables (host-computed in double): per destination column x0, x1, wx0, wx1; per destination row y0, y1, wy0, wy1
struct FlowResizeTab {
    const int32_t *x0, *x1, *y0, *y1;
    const float *wx0, *wx1, *wy0, *wy1;
};

// the working planes of the level being refined (each plane rows x cols, row-major)
struct FlowLevelBufs {
    float *u, *v, *du, *dv, *avg;
    float* d[FLOW_NDERIV];
    float* c[FLOW_NCOEF];
};

// the finished coarser level (u + du, v + dv is its flow); u == nullptr on the coarsest level
struct FlowCoarse {
    const float *u, *v, *du, *dv;
    int rows, cols;
    FlowResizeTab tab;  // coarse -> this level
};

struct FlowConsts {
    float alpha, delta, gamma;  // 4 alpha, delta / 3, gamma / 3
};

struct FlowSorArgs {
    const float* c[FLOW_NCOEF];
    const float *du_in, *dv_in;
    float *du_out, *dv_out;
    int rows, cols, halo, tiles_x, nit;
    float om, om1;  // omega, 1 - omega
};

hipError_t flow_presmooth(hipStream_t s, const uint8_t* img1, const uint8_t* img2, int rows, int cols, int channels, const float* taps, int radius,
                          float* tmp1, float* tmp2, float* out1, float* out2);
hipError_t flow_pyr_down(hipStream_t s, const float* src1, const float* src2, int scols, const FlowResizeTab& tab, int rows, int cols, float* dst1,
                         float* dst2);
hipError_t flow_level_entry(hipStream_t s, const FlowLevelBufs& L, const float* i1, const float* i2, int rows, int cols, const FlowCoarse& C,
                            float scale);
hipError_t flow_coef(hipStream_t s, const FlowLevelBufs& L, int rows, int cols, const FlowConsts& k);
hipError_t flow_sor(hipStream_t s, const FlowSorArgs& a, int tiles);
hipError_t flow_output(hipStream_t s, const FlowLevelBufs& L, int rows, int cols, double* flow);

// ---- batches of consecutive pairs (flow_seq_kernels.hip; DESIGN section 12, "Sequences") ------------------------------------------
// A batch of n <= kFlowSeqMaxPairs pairs reads n + 1 frames; per-frame planes at base + frame * pstride (pyramids) or * stride (the
// blur's temporary), per-pair planes at base + pair * stride.  The frames and the output fields are kernel-argument tables.
constexpr int kFlowSeqMaxPairs = 32;
struct FlowFramePtrs {
    const uint8_t* p[kFlowSeqMaxPairs + 1];
};
struct FlowOutPtrs {
    double* p[kFlowSeqMaxPairs];
};

hipError_t flow_seq_presmooth(hipStream_t s, const FlowFramePtrs& img, int nframes, int rows, int cols, int channels, const float* taps, int radius,
                              float* tmp, size_t stride, float* pyr, size_t pstride);
hipError_t flow_seq_pyr_down(hipStream_t s, const float* src, int scols, const FlowResizeTab& tab, int rows, int cols, float* dst, size_t pstride,
                             int nframes);
hipError_t flow_seq_level_entry(hipStream_t s, const FlowLevelBufs& L, size_t stride, const float* pyr_l, size_t pstride, int rows, int cols,
                                const FlowCoarse& C, float scale, int npairs);
hipError_t flow_seq_coef(hipStream_t s, const FlowLevelBufs& L, size_t stride, int rows, int cols, const FlowConsts& k, int npairs);
hipError_t flow_seq_sor(hipStream_t s, const FlowSorArgs& a, size_t stride, int tiles, int npairs);
hipError_t flow_seq_output(hipStream_t s, const FlowLevelBufs& L, size_t stride, int rows, int cols, const FlowOutPtrs& out, int npairs);

}  // namespace rsdsfm
