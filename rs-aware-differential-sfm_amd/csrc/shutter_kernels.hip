// shutter_kernels.hip -- the synthetic shutter's temporal integrator on MI355X (gfx950, wave64): include/rsdsfm_shutter.h, defined by
// tests/shutter_spec_numpy.py and reproduced bit for bit.  Integer arithmetic only; every value goes to memory through ordinary stores and atomicAdd.
//   shutter_accumulate_kernel<CH, FIRST, LAST>  retime_merge_kernel's shape: the planes are flat arrays; grid-stride under a grid of at most 1024
//                               workgroups, a thread owns 4 consecutive pixels.  The sample's mask dword first; the image's CH dwords only when some
//                               byte of it is set.  A pixel's cell is CH + 1 uint16 [sums, n]: the thread's four cells are 32 B (BGR) or 16 B
//                               (gray), moved as 16-byte accesses.  FIRST: the cells are not read (their previous contents never show).  Neither
//                               FIRST nor LAST and an empty mask word: the cells are neither read nor written.  LAST: the cells are not written;
//                               out_c = (2 s_c + n) / (2 n) (a true unsigned divide, n <= 64 and 2 s_c + n <= 32 704) and mask 1 where
//                               n >= min_samples, else 0 / 0; the image's CH dwords, the mask's and the coverage plane's dword are written whole:
//                               every byte of the outputs is written, no preset.  The last rows cols % 4 pixels byte by byte (the byte tail).
//                               A mid sample of a BGR frame moves 1 + 3 + 8 + 8 = 20 B per pixel where its mask is set.
//                               The three counters [unset, partial, full] (block_counts_add, image_tile_device.hpp: 3 072 atomicAdd at most in
//                               all), only in LAST and only when a counter pointer was passed.  The cells here always start on 16 bytes and the
//                               tail goes halfword by halfword, so this kernel keeps its own cell access and output stores.
#include <algorithm>

#include "image_tile_device.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"
#include "shutter.hpp"

namespace rsdsfm {

namespace {

// one pixel resolved: n and its CH sums -> the CH output bytes (0 where n < min_samples); returns 1 where the pixel is set
template <int CH>
__device__ __forceinline__ unsigned resolve_pixel(unsigned n, const unsigned* s, unsigned min_samples, unsigned* v) {
    const bool ok = n >= min_samples;  // min_samples >= 1: n != 0 where ok
    const unsigned den = ok ? 2u * n : 1u;
#pragma unroll
    for (int c = 0; c < CH; ++c) v[c] = ok ? (2u * s[c] + n) / den : 0u;  // round half up
    return ok ? 1u : 0u;
}

template <int CH, bool FIRST, bool LAST>
__device__ __forceinline__ void shutter_accumulate_body(const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask, unsigned short* __restrict__ cells,
                                                        int npix, unsigned nsamples, unsigned min_samples, unsigned char* __restrict__ out,
                                                        unsigned char* __restrict__ mask_out, unsigned char* __restrict__ coverage,
                                                        unsigned long long* __restrict__ counts) {
    constexpr int H = CH + 1;      // halfwords per cell
    constexpr int W = 4 * H / 2;   // dwords of a thread's four cells: 8 (BGR) or 4 (gray)
    unsigned n3[3] = {0u, 0u, 0u};  // [unset, partial, full]; at most 4 per step and 2^28 / 4 steps in all: no overflow
    const int64_t stride = (int64_t)gridDim.x * kBP * 4;
    for (int64_t q0 = ((int64_t)blockIdx.x * kBP + threadIdx.x) * 4; q0 < npix; q0 += stride) {
        const int p0 = (int)q0;
        if (p0 + 4 <= npix) {  // p0 % 4 == 0: p0 and CH * p0 bytes are 4-byte aligned, the cells' 2 H p0 bytes 16-byte aligned from their base
            const unsigned m = bytes_set(*reinterpret_cast<const unsigned*>(mask + p0));
            if (!FIRST && !LAST && m == 0u) continue;  // nothing to add: the cells are neither read nor written
            unsigned iw[CH], cw[W];
#pragma unroll
            for (int d = 0; d < CH; ++d) iw[d] = m ? reinterpret_cast<const unsigned*>(image + (int64_t)CH * p0)[d] : 0u;  // an empty word's image is not read
            Cells16* cp = (FIRST && LAST) ? nullptr : reinterpret_cast<Cells16*>(cells + (int64_t)H * p0);
#pragma unroll
            for (int k = 0; k < W / 4; ++k) {
                Cells16 v = {0u, 0u, 0u, 0u};
                if (!FIRST) v = cp[k];
#pragma unroll
                for (int i = 0; i < 4; ++i) cw[4 * k + i] = v[i];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned set = (m >> (8 * j)) & 1u;
                unsigned v[H];
#pragma unroll
                for (int c = 0; c < CH; ++c) v[c] = set ? byte_of(iw, CH * j + c) : 0u;  // bytes under an empty mask byte do not show
                v[CH] = set;
#pragma unroll
                for (int h = 0; h < H; ++h) cw[(H * j + h) >> 1] += v[h] << (16 * ((H * j + h) & 1));  // no halfword overflows: n <= 64, sums <= 16 320
            }
            if (!LAST) {
#pragma unroll
                for (int k = 0; k < W / 4; ++k) cp[k] = Cells16{cw[4 * k], cw[4 * k + 1], cw[4 * k + 2], cw[4 * k + 3]};
            } else {
                unsigned ow[CH], mw = 0u, cov = 0u;
#pragma unroll
                for (int d = 0; d < CH; ++d) ow[d] = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    unsigned s[CH], v[CH];
#pragma unroll
                    for (int c = 0; c < CH; ++c) s[c] = half_of(cw, H * j + c);
                    const unsigned n = half_of(cw, H * j + CH);
                    const unsigned ok = resolve_pixel<CH>(n, s, min_samples, v);
#pragma unroll
                    for (int c = 0; c < CH; ++c) ow[(CH * j + c) >> 2] |= v[c] << (8 * ((CH * j + c) & 3));
                    mw |= ok << (8 * j);
                    cov |= (n & 0xffu) << (8 * j);
                    n3[0] += 1u - ok;
                    n3[1] += (ok && n != nsamples) ? 1u : 0u;
                    n3[2] += n == nsamples ? 1u : 0u;
                }
#pragma unroll
                for (int d = 0; d < CH; ++d) reinterpret_cast<unsigned*>(out + (int64_t)CH * p0)[d] = ow[d];
                *reinterpret_cast<unsigned*>(mask_out + p0) = mw;
                if (coverage) *reinterpret_cast<unsigned*>(coverage + p0) = cov;
            }
        } else {
            for (int p = p0; p < npix; ++p) {
                const bool set = mask[p] != 0;
                if (!FIRST && !LAST && !set) continue;
                unsigned s[CH], v[CH];
                unsigned short* cell = (FIRST && LAST) ? nullptr : cells + (int64_t)H * p;
                unsigned n = FIRST ? 0u : cell[CH];
#pragma unroll
                for (int c = 0; c < CH; ++c) s[c] = (FIRST ? 0u : cell[c]) + (set ? image[(int64_t)CH * p + c] : 0u);
                n += set ? 1u : 0u;
                if (!LAST) {
#pragma unroll
                    for (int c = 0; c < CH; ++c) cell[c] = (unsigned short)s[c];
                    cell[CH] = (unsigned short)n;
                } else {
                    const unsigned ok = resolve_pixel<CH>(n, s, min_samples, v);
#pragma unroll
                    for (int c = 0; c < CH; ++c) out[(int64_t)CH * p + c] = (unsigned char)v[c];
                    mask_out[p] = (unsigned char)ok;
                    if (coverage) coverage[p] = (unsigned char)n;
                    n3[0] += 1u - ok;
                    n3[1] += (ok && n != nsamples) ? 1u : 0u;
                    n3[2] += n == nsamples ? 1u : 0u;
                }
            }
        }
    }
    if constexpr (LAST) block_counts_add<3>(n3, counts);
}

}  // namespace

// grid-stride over groups of 4 pixels, block kBP.  Not LAST: cells += the sample (FIRST: cells = the sample).  LAST: out, mask_out and coverage (may
// be NULL) are written whole from cells + the sample; counts[0 .. 2] += [unset, partial, full]
template <int CH, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBP) void shutter_accumulate_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask,
                                                                unsigned short* __restrict__ cells, int npix, unsigned nsamples, unsigned min_samples,
                                                                unsigned char* __restrict__ out, unsigned char* __restrict__ mask_out,
                                                                unsigned char* __restrict__ coverage, unsigned long long* __restrict__ counts) {
    shutter_accumulate_body<CH, FIRST, LAST>(image, mask, cells, npix, nsamples, min_samples, out, mask_out, coverage, counts);
}

// ---------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------
int shutter_accumulate_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, int channels, int rows, int cols, uint16_t* d_cells, bool first, bool last,
                              int nsamples, int min_samples, unsigned char* d_image_out, unsigned char* d_mask_out, unsigned char* d_coverage, int64_t* d_counts3) {
    if (last && d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    const int npix = rows * cols;  // rows, cols <= 16384
    const int64_t nb = ((int64_t)npix + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    const dim3 grid((unsigned)std::min<int64_t>(nb, kShutterGridMax));
    using Kernel = void (*)(const unsigned char*, const unsigned char*, unsigned short*, int, unsigned, unsigned, unsigned char*, unsigned char*, unsigned char*,
                            unsigned long long*);
    static const Kernel kernels[2][2][2] = {
        {{shutter_accumulate_kernel<1, false, false>, shutter_accumulate_kernel<1, false, true>},
         {shutter_accumulate_kernel<1, true, false>, shutter_accumulate_kernel<1, true, true>}},
        {{shutter_accumulate_kernel<3, false, false>, shutter_accumulate_kernel<3, false, true>},
         {shutter_accumulate_kernel<3, true, false>, shutter_accumulate_kernel<3, true, true>}}};
    // the outputs are passed only to the instances that write them
    hipLaunchKernelGGL(kernels[channels == 3][first][last], grid, dim3(kBP), 0, c->stream, d_image, d_mask, d_cells, npix, (unsigned)nsamples, (unsigned)min_samples,
                       last ? d_image_out : nullptr, last ? d_mask_out : nullptr, last ? d_coverage : nullptr,
                       last ? reinterpret_cast<unsigned long long*>(d_counts3) : nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
