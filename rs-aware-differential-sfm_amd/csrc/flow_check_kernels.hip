// flow_check_kernels.hip -- the forward-backward flow check on MI355X (gfx950): include/rsdsfm_flow_check.h, defined by
// tests/flow_check_spec_numpy.py and reproduced bit for bit (float64 arithmetic, one rounding per operation, -ffp-contract=off; the
// numbered steps below are the spec's).  No per-pixel model code: both library builds compile it the same way.
//
// One streaming pass, one lane per pixel over the flat pixel index, pair index in blockIdx.z (a clip batch is one launch).  A lane reads
// its forward vector (16 B, coalesced), gathers the four 16 B taps of the backward field around its landing point (a few pixels away: L2
// hits), writes the masked vector (16 B) and the residual (8 B) where they are asked for, and the wave packs its 64 mask bits into sixteen
// 32-bit words (a wave starts at a multiple of 64 pixels; the last 1 - 3 pixels of a field go out as bytes).  The consistent pixels are
// counted per wave from the ballot, per workgroup in LDS, and added to the pair's counter with one integer atomic per workgroup: exact
// and independent of order.  No private segment.
//
// Algorithmic HBM traffic per pixel: 16 B + 16 B read (the taps re-read the backward field through the caches), 1 B mask + 16 B masked
// field (+ 8 B residual) written = 49 B (57 B).
#include <math.h>

#include "flow_check.hpp"

namespace rsdsfm {

namespace {

constexpr int kCB = 256;  // threads of a workgroup: 4 waves

__device__ __forceinline__ double lerp(double a, double b, double t) { return a + t * (b - a); }

}  // namespace

// grid: (ceil(rows * cols / kCB), 1, pairs)
__global__ __launch_bounds__(kCB) void flow_check_kernel(FlowCheckPtrs t, int rows, int cols, int npix, double a1, double a2) {
    __shared__ int s_count;
    const int pair = blockIdx.z;
    const double* fwd = t.fwd[pair];  // (masked may be fwd: a lane reads its own pixel before it writes it)
    const double* bwd = t.bwd[pair];
    unsigned char* mask = t.mask[pair];
    double* masked = t.masked[pair];
    double* resid = t.resid[pair];
    if (threadIdx.x == 0) s_count = 0;
    __syncthreads();
    const int idx = (int)blockIdx.x * kCB + (int)threadIdx.x;
    bool keep = false;
    if (idx < npix) {
        const int i = idx / cols, j = idx - i * cols;
        const double u = fwd[2 * (size_t)idx], v = fwd[2 * (size_t)idx + 1];
        const double px = (double)j + u, py = (double)i + v;                                                         // 1
        const bool inside = px >= 0.0 && px <= (double)(cols - 1) && py >= 0.0 && py <= (double)(rows - 1);
        double r = INFINITY;
        if (inside) {
            const double x0 = fmin(floor(px), (double)(cols - 2)), y0 = fmin(floor(py), (double)(rows - 2));         // 2
            const double ax = px - x0, ay = py - y0;
            const double* r0 = bwd + 2 * ((size_t)(int)y0 * (size_t)cols + (size_t)(int)x0);  // taps (y0, x0) .. (y0 + 1, x0 + 1): inside the field
            const double* r1 = r0 + 2 * (size_t)cols;
            const double bu = lerp(lerp(r0[0], r0[2], ax), lerp(r1[0], r1[2], ax), ay);                              // 3
            const double bv = lerp(lerp(r0[1], r0[3], ax), lerp(r1[1], r1[3], ax), ay);
            const double rr = (u + bu) * (u + bu) + (v + bv) * (v + bv);                                             // 4
            const double bound = a1 * ((u * u + v * v) + (bu * bu + bv * bv)) + a2;                                  // 5
            keep = rr <= bound;                                                                                      // 6
            if (rr < INFINITY) r = rr;                                                                               // 7 (rr >= 0 or NaN)
        }
        if (masked) masked[2 * (size_t)idx] = keep ? u : 0.0, masked[2 * (size_t)idx + 1] = keep ? v : 0.0;          // 8
        if (resid) resid[idx] = r;
    }
    // the wave's 64 mask bits: lane 4 m packs pixels idx .. idx + 3 into one word (idx is a multiple of 4 there)
    const unsigned long long bits = __ballot(keep);
    const int lane = (int)threadIdx.x & 63;
    if ((lane & 3) == 0 && idx < npix) {
        const unsigned nib = (unsigned)(bits >> lane) & 0xFu;
        if (idx + 3 < npix) {
            *reinterpret_cast<unsigned*>(mask + idx) = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
        } else {
            for (int k = 0; idx + k < npix; ++k) mask[idx + k] = (unsigned char)((nib >> k) & 1u);
        }
    }
    if (lane == 0) atomicAdd(&s_count, (int)__popcll(bits));                                                         // 9
    __syncthreads();
    if (threadIdx.x == 0 && t.count[pair] && s_count) atomicAdd(reinterpret_cast<unsigned long long*>(t.count[pair]), (unsigned long long)s_count);
}

hipError_t flow_check_launch(hipStream_t s, const FlowCheckPtrs& t, int npairs, int rows, int cols, double a1, double a2) {
    const int npix = rows * cols;  // <= 2^28
    hipLaunchKernelGGL(flow_check_kernel, dim3((unsigned)((npix + kCB - 1) / kCB), 1u, (unsigned)npairs), dim3(kCB), 0, s, t, rows, cols, npix, a1, a2);
    return hipGetLastError();
}

}  // namespace rsdsfm
