// retime_kernels.hip -- the retimer's merge on MI355X (gfx950, wave64): include/rsdsfm_retime.h, defined by tests/retime_spec_numpy.py and
// reproduced bit for bit.  Integer arithmetic only; every value goes to memory through ordinary stores and atomicAdd.
//   retime_merge_kernel<CH, HAS_B>  the planes are flat arrays; grid-stride under a grid of at most 1024 workgroups, a thread owns 4 consecutive
//                               pixels: both masks' dwords first (2 B per pixel).  Both 0: zeros are written and no image is read.  Else layer
//                               a's CH dwords only when some byte of a's mask is set, and layer b's likewise -- where one layer is empty over the
//                               4 pixels the other is copied and the empty one is not read.  The image's CH dwords, the mask's and the source
//                               plane's dword are written whole: every byte of the outputs is written, no preset.  BGR with the source plane:
//                               8 B read and 5 B written per pixel where both layers are set.  The last rows cols % 4 pixels byte by byte (the
//                               byte tail).  HAS_B = false: b absent everywhere (one source), its pointers are not touched.
//                               The five counters (block_counts_add, image_tile_device.hpp: 5 120 atomicAdd at most in all), only when a
//                               counter pointer was passed.
#include <algorithm>

#include "image_tile_device.hpp"
#include "rectify_dense_device.hpp"
#include "retime.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace {

// one pixel: the source byte (RSDSFM_RETIME_*) from the two mask bits and the two pixels' channels, and the output channels
template <int CH>
__device__ __forceinline__ unsigned merge_pixel(bool aj, bool bj, const unsigned* va, const unsigned* vb, unsigned w, unsigned thr, unsigned* v) {
    unsigned d = 0u;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const unsigned diff = va[c] > vb[c] ? va[c] - vb[c] : vb[c] - va[c];
        d = diff > d ? diff : d;
    }
    const unsigned s = (aj && bj) ? (d <= thr ? (unsigned)RSDSFM_RETIME_DISSOLVED : w > 32768u ? (unsigned)RSDSFM_RETIME_CONFLICT_B : (unsigned)RSDSFM_RETIME_CONFLICT_A)
                       : aj       ? (unsigned)RSDSFM_RETIME_FROM_A
                       : bj       ? (unsigned)RSDSFM_RETIME_FROM_B
                                  : (unsigned)RSDSFM_RETIME_NONE;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const unsigned mix = (va[c] * (65536u - w) + vb[c] * w + 32768u) >> 16;  // < 2^8 2^16 + 2^15: no overflow
        v[c] = s == RSDSFM_RETIME_DISSOLVED ? mix : (s == RSDSFM_RETIME_FROM_A || s == RSDSFM_RETIME_CONFLICT_A) ? va[c] : s == RSDSFM_RETIME_NONE ? 0u : vb[c];
    }
    return s;
}

template <int CH, bool HAS_B>
__device__ __forceinline__ void retime_merge_body(const unsigned char* __restrict__ image_a, const unsigned char* __restrict__ mask_a,
                                                  const unsigned char* __restrict__ image_b, const unsigned char* __restrict__ mask_b, int npix, unsigned w,
                                                  unsigned thr, unsigned char* __restrict__ out, unsigned char* __restrict__ mask, unsigned char* __restrict__ source,
                                                  unsigned long long* __restrict__ counts) {
    unsigned n[5] = {0u, 0u, 0u, 0u, 0u};  // at most 4 per step and 2^28 / 4 steps in all: no overflow
    const int64_t stride = (int64_t)gridDim.x * kBP * 4;
    for (int64_t q0 = ((int64_t)blockIdx.x * kBP + threadIdx.x) * 4; q0 < npix; q0 += stride) {
        const int p0 = (int)q0;
        if (p0 + 4 <= npix) {  // p0 % 4 == 0: p0 and CH * p0 bytes are 4-byte aligned
            const unsigned a = bytes_set(*reinterpret_cast<const unsigned*>(mask_a + p0));
            const unsigned b = HAS_B ? bytes_set(*reinterpret_cast<const unsigned*>(mask_b + p0)) : 0u;
            unsigned* op = reinterpret_cast<unsigned*>(out + (int64_t)CH * p0);
            unsigned ow[CH], sw = 0u;
#pragma unroll
            for (int d = 0; d < CH; ++d) ow[d] = 0u;
            if ((a | b) != 0u) {
                unsigned ia[CH], ib[CH];
#pragma unroll
                for (int d = 0; d < CH; ++d) {
                    ia[d] = a ? reinterpret_cast<const unsigned*>(image_a + (int64_t)CH * p0)[d] : 0u;  // an empty layer is not read
                    ib[d] = (HAS_B && b) ? reinterpret_cast<const unsigned*>(image_b + (int64_t)CH * p0)[d] : 0u;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    unsigned va[CH], vb[CH], v[CH];
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        va[c] = byte_of(ia, CH * j + c);
                        vb[c] = byte_of(ib, CH * j + c);
                    }
                    const unsigned s = merge_pixel<CH>((a >> (8 * j)) & 1u, (b >> (8 * j)) & 1u, va, vb, w, thr, v);
#pragma unroll
                    for (int c = 0; c < CH; ++c) ow[(CH * j + c) >> 2] |= v[c] << (8 * ((CH * j + c) & 3));
                    sw |= s << (8 * j);
#pragma unroll
                    for (int k = 0; k < 5; ++k) n[k] += (s > 4u ? 4u : s) == (unsigned)k ? 1u : 0u;
                }
            } else {
                n[0] += 4u;
            }
#pragma unroll
            for (int d = 0; d < CH; ++d) op[d] = ow[d];
            *reinterpret_cast<unsigned*>(mask + p0) = a | b;
            if (source) *reinterpret_cast<unsigned*>(source + p0) = sw;
        } else {
            for (int p = p0; p < npix; ++p) {
                const bool aj = mask_a[p] != 0, bj = HAS_B && mask_b[p] != 0;
                unsigned va[CH], vb[CH], v[CH];
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    va[c] = aj ? image_a[(int64_t)CH * p + c] : 0u;
                    vb[c] = bj ? image_b[(int64_t)CH * p + c] : 0u;
                }
                const unsigned s = merge_pixel<CH>(aj, bj, va, vb, w, thr, v);
#pragma unroll
                for (int c = 0; c < CH; ++c) out[(int64_t)CH * p + c] = (unsigned char)v[c];
                mask[p] = (aj || bj) ? 1 : 0;
                if (source) source[p] = (unsigned char)s;
#pragma unroll
                for (int k = 0; k < 5; ++k) n[k] += (s > 4u ? 4u : s) == (unsigned)k ? 1u : 0u;
            }
        }
    }
    block_counts_add<5>(n, counts);
}

}  // namespace

// grid-stride over groups of 4 pixels, block kBP: out, mask and source (may be NULL) are written whole; counts[0 .. 4] += [none, a only, b only,
// dissolved, conflict]
template <int CH, bool HAS_B>
__global__ __launch_bounds__(kBP) void retime_merge_kernel(const unsigned char* __restrict__ image_a, const unsigned char* __restrict__ mask_a,
                                                          const unsigned char* __restrict__ image_b, const unsigned char* __restrict__ mask_b, int npix, unsigned w,
                                                          unsigned thr, unsigned char* __restrict__ out, unsigned char* __restrict__ mask,
                                                          unsigned char* __restrict__ source, unsigned long long* __restrict__ counts) {
    retime_merge_body<CH, HAS_B>(image_a, mask_a, image_b, mask_b, npix, w, thr, out, mask, source, counts);
}

// ---------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------
int retime_merge_launch(Ctx* c, const unsigned char* d_image_a, const unsigned char* d_mask_a, const unsigned char* d_image_b, const unsigned char* d_mask_b,
                        int channels, int rows, int cols, int weight_q16, int threshold, unsigned char* d_image_out, unsigned char* d_mask_out,
                        unsigned char* d_source, int64_t* d_counts5) {
    if (d_counts5) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts5, 0, 5 * sizeof(int64_t), c->stream));
    const int npix = rows * cols;  // rows, cols <= 16384
    const int64_t nb = ((int64_t)npix + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    const dim3 grid((unsigned)std::min<int64_t>(nb, kRetimeGridMax));
    const bool has_b = d_mask_b != nullptr;
    auto kernel = channels == 3 ? (has_b ? retime_merge_kernel<3, true> : retime_merge_kernel<3, false>) : (has_b ? retime_merge_kernel<1, true> : retime_merge_kernel<1, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kBP), 0, c->stream, d_image_a, d_mask_a, d_image_b, d_mask_b, npix, (unsigned)weight_q16, (unsigned)threshold, d_image_out,
                       d_mask_out, d_source, reinterpret_cast<unsigned long long*>(d_counts5));
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
