// stabilize_fill_kernels.hip -- one candidate of the stabiliser's border fill on MI355X (gfx950): include/rsdsfm_stabilize_fill.h, defined
// by tests/stabilize_fill_spec_numpy.py and reproduced bit for bit (float64 arithmetic, one rounding per operation, -ffp-contract=off).
// Stage A (the inverse-depth fill) is the dense rectifier's launches and stage B the stabiliser's map kernel with the neighbour's pose,
// both unchanged (rectify_dense_kernels.hip, stabilize_kernels.hip); this file has what stands in stage C's place:
//   stabilize_fill_warp_kernel / stabilize_fill_warp_gray_kernel (3 / 1 channels)
//       warp_body's structure (rectify_dense_device.hpp) -- a thread owns 4 consecutive pixels, 12 bytes = 3 dwords of the image and one
//       dword of the mask, the last fewer-than-4 pixels of the frame byte by byte -- but the thread loads the mask's dword FIRST: 0x01010101
//       (the common case, away from the border) and it is done, at 1 B read per pixel.  Else warp_pixel<CH> for the pixels whose byte is 0,
//       so that a filled pixel has by construction the bytes stage C would write, and the image, mask and source dwords written back merged
//       with what was there (the image's dwords are read only when some of the 4 pixels are kept).  A thread reads and writes only its own
//       4 pixels of the in-out planes and samples only the neighbour's image and the displacement plane: no race.  The number of pixels
//       taken: a sum per thread, shuffles, LDS, one 64-bit integer atomicAdd per workgroup -- exact and independent of scheduling.
#include <algorithm>

#include "rectify_dense.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_fill.hpp"

namespace rsdsfm {

namespace {

template <int CH>
__device__ __forceinline__ void fill_warp_body(const unsigned char* __restrict__ img, const float2* __restrict__ disp, const double* __restrict__ top, int rows,
                                               int cols, int iterations, unsigned sid, unsigned char* __restrict__ out, unsigned char* __restrict__ mask,
                                               unsigned char* __restrict__ source, unsigned long long* __restrict__ count) {
    __shared__ unsigned s_wave[kBP / 64];
    const int npix = rows * cols;  // rows, cols <= 16384
    unsigned n = 0;                // at most 4 per step and 2^28 / 4 steps in all: no overflow
    if (*top != 0.0) {             // the 1 x 1 level: 0 = the candidate has no valid depth = it offers nothing (uniform)
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
                    if (((old >> (8 * j)) & 0xffu) == 0u) t[j] = warp_pixel<CH>(img, disp, rows, cols, iterations, p0 + j, v + CH * j);
                }
                const unsigned take = t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24);  // 1 in the bytes of the pixels taken
                if (take == 0u) continue;
                n += __popc(take);
                unsigned* dst = reinterpret_cast<unsigned*>(out + (int64_t)CH * p0);
                if (take == 0x01010101u) {  // nothing of the 4 pixels is kept: no read
#pragma unroll
                    for (int d = 0; d < CH; ++d) dst[d] = v[4 * d] | (v[4 * d + 1] << 8) | (v[4 * d + 2] << 16) | (v[4 * d + 3] << 24);
                    if (source) *reinterpret_cast<unsigned*>(source + p0) = sid * 0x01010101u;
                } else {  // (v is 0 in the bytes of the pixels not taken)
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
                        if (warp_pixel<CH>(img, disp, rows, cols, iterations, p0 + j, v)) {
#pragma unroll
                            for (int c = 0; c < CH; ++c) out[(int64_t)CH * (p0 + j) + c] = (unsigned char)v[c];
                            mask[p0 + j] = 1;
                            if (source) source[p0 + j] = (unsigned char)sid;
                            ++n;
                        }
                    }
            }
        }
    }
    if (!count) return;  // (uniform)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x / 64] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kBP / 64; ++w) total += s_wave[w];
        if (total) atomicAdd(count, (unsigned long long)total);
    }
}

}  // namespace

// grid-stride over groups of 4 pixels, block kBP: as rectify_dense_warp_kernel.  mask, out and source are in-out; *count += the pixels taken
__global__ __launch_bounds__(kBP) void stabilize_fill_warp_kernel(const unsigned char* __restrict__ img, const float2* __restrict__ disp,
                                                                 const double* __restrict__ top, int rows, int cols, int iterations, unsigned sid,
                                                                 unsigned char* __restrict__ out, unsigned char* __restrict__ mask,
                                                                 unsigned char* __restrict__ source, unsigned long long* __restrict__ count) {
    fill_warp_body<3>(img, disp, top, rows, cols, iterations, sid, out, mask, source, count);
}

__global__ __launch_bounds__(kBP) void stabilize_fill_warp_gray_kernel(const unsigned char* __restrict__ img, const float2* __restrict__ disp,
                                                                      const double* __restrict__ top, int rows, int cols, int iterations, unsigned sid,
                                                                      unsigned char* __restrict__ out, unsigned char* __restrict__ mask,
                                                                      unsigned char* __restrict__ source, unsigned long long* __restrict__ count) {
    fill_warp_body<1>(img, disp, top, rows, cols, iterations, sid, out, mask, source, count);
}

// ---------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------
int stabilize_fill_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img_n, int channels, const double* d_depth_cm, const double* d_R, const double* d_t,
                          double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp, int source_id,
                          unsigned char* d_out, unsigned char* d_mask, unsigned char* d_source, int64_t* d_filled) {
    const double* top = nullptr;
    const int rc = rectify_dense_launch_fill(c, ws, d_depth_cm, rows, cols, &top);
    if (rc != RSDSFM_OK) return rc;
    const DensePlan p = rectify_dense_plan(rows, cols);
    const dim3 tiles((cols + kTX - 1) / kTX, (rows + kTY - 1) / kTY);
    hipLaunchKernelGGL(stabilize_map_kernel, tiles, dim3(kCB), 0, c->stream, d_depth_cm, ws.d_pyr, p.h[0], p.w[0], d_R, d_t, fx, fy, cx, cy, q5_mode == 0 ? fx : fy, rows,
                       cols, mode, vp, ws.d_disp, (double*)nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    if (d_filled) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_filled, 0, sizeof(int64_t), c->stream));
    const int64_t npix = (int64_t)rows * cols;
    const int64_t nb = (npix + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    hipLaunchKernelGGL(channels == 3 ? stabilize_fill_warp_kernel : stabilize_fill_warp_gray_kernel, dim3((unsigned)std::min<int64_t>(nb, 65536)), dim3(kBP), 0, c->stream,
                       d_img_n, ws.d_disp, top, rows, cols, iterations, (unsigned)source_id, d_out, d_mask, d_source, reinterpret_cast<unsigned long long*>(d_filled));
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
