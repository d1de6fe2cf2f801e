// deblur_kernels.hip -- the sharpness transfer's two kernels on MI355X (gfx950, wave64): include/rsdsfm_deblur.h, defined by
// tests/deblur_spec_numpy.py and reproduced bit for bit.  Integer arithmetic only; every value goes to memory through ordinary stores and atomicAdd.
// Both run on the 16 x 64 tile of image_tile_device.hpp (the plane reads, the LDS layout and its bank argument, the cells, the output group and
// the counters are described there), and in both every workgroup computes the CH gains itself from the 8-word record (seam_gain, threads
// 0 .. CH - 1, through LDS): no host wait behind the sums kernel.
//   deblur_sharpness_kernel<CH>   the record T = [pairs, A_R, A_L, 0].  The two mask dwords first; R's and L's CH dwords only where some pixel
//                               has both masks set.  Per pixel the packed dword (v << 20) | (Y_R << 10) | Y_L -- 1 + 10 + 10 bits, Y <= 765 --
//                               goes to the tile's LDS plane, 0 for a pixel outside the frame or without both masks.  Of the halo only the
//                               column to the right and the row below are formed (80 of the 164 halo threads, each its own pixel, gains
//                               included, masks first).  A thread then takes the pairs of its four pixels: the right neighbours are its own
//                               registers and one LDS dword, the lower neighbours four LDS dwords, read as four 8-byte reads at
//                               [ty + 2][4 g .. 4 g + 5] and [ty + 1][4 g + 4, 4 g + 5] -- tile_sum3x3's addresses, so its bank argument holds
//                               (64 banks for an 8-byte read; as 4-byte reads, 32 banks, threads g and g + 8 would collide).  The three sums go
//                               through block_counts_add<3>: a workgroup's largest sum is 2 * 1024 * 765^2 = 1 198 540 800 < 2^32.
//   deblur_accumulate_kernel<CH, FIRST, LAST>  the denoise's structure.  One thread computes tau from T (one 64-bit integer division) and shares
//                               it through LDS with the gains.  A launch with tau == 0 that is neither FIRST nor LAST returns there: it has read
//                               the two records and nothing else.  With tau == 0 a FIRST or LAST launch runs as if no layer were given (u = 0
//                               everywhere).  Stage 1: the packed dword (v << 16) | (Y_R - Y_L + 765) goes to LDS.  Stage 2: the sum of the
//                               3 x 3 packed dwords holds the count in the high half and sum + 765 count in the low half (<= 9 * 1530 = 13 770:
//                               the field does not carry); D = |low - 765 count|, w = 16 - min(16, 16 D / (h CH count)) where v (gate_mode 1:
//                               16), u = (w tau + 8) >> 4.  The cells, the outputs and the counters as the denoise's.
// The bodies live in deblur_sharpness_body.hpp and deblur_device.hpp, which deblur_bands_kernels.hip (a tau per band of rows) shares.
#include <algorithm>

#include "deblur.hpp"
#include "deblur_device.hpp"
#include "image_tile_device.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  T[0 .. 2] += [pairs, A_R, A_L] of the workgroup's tile (T zeroed by the caller)
template <int CH>
__global__ __launch_bounds__(kBP) void deblur_sharpness_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                              const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                              const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode,
                                                              unsigned long long* __restrict__ T) {
#include "deblur_sharpness_body.hpp"
}

template <int CH, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBP) void deblur_accumulate_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                               const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                               const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode, unsigned strength,
                                                               const unsigned long long* __restrict__ sharp, int margin, long long min_pairs, int gate_mode,
                                                               unsigned short* __restrict__ cells, unsigned char* __restrict__ out,
                                                               unsigned char* __restrict__ mask_out, unsigned char* __restrict__ weight,
                                                               unsigned long long* __restrict__ counts) {
    deblur_accumulate_body<CH, FIRST, LAST, false>(ref, rmask, layer, lmask, rows, cols, sums, min_overlap, gain_mode, strength, sharp, 0, 0, margin, min_pairs, gate_mode,
                                                   cells, out, mask_out, weight, counts);
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int deblur_sharpness_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                            int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, unsigned long long* d_sharp4) {
    RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_sharp4, 0, 4 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(channels == 3 ? deblur_sharpness_kernel<3> : deblur_sharpness_kernel<1>, tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_ref, d_rmask, d_layer,
                       d_lmask, rows, cols, d_sums, (long long)min_overlap, gain_mode, d_sharp4);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int deblur_accumulate_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                             int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int strength, const unsigned long long* d_sharp4,
                             int margin, int64_t min_pairs, int gate_mode, uint16_t* d_cells, bool first, bool last, unsigned char* d_image_out, unsigned char* d_mask_out,
                             unsigned char* d_weight, int64_t* d_counts3) {
    if (last && d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, int, int, const unsigned long long*, long long, int,
                            unsigned, const unsigned long long*, int, long long, int, unsigned short*, unsigned char*, unsigned char*, unsigned char*, unsigned long long*);
    static const Kernel kernels[2][2][2] = {
        {{deblur_accumulate_kernel<1, false, false>, deblur_accumulate_kernel<1, false, true>},
         {deblur_accumulate_kernel<1, true, false>, deblur_accumulate_kernel<1, true, true>}},
        {{deblur_accumulate_kernel<3, false, false>, deblur_accumulate_kernel<3, false, true>},
         {deblur_accumulate_kernel<3, true, false>, deblur_accumulate_kernel<3, true, true>}}};
    // the outputs are passed only to the instances that write them
    hipLaunchKernelGGL(kernels[channels == 3][first][last], tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_ref, d_rmask, d_layer, d_lmask, rows, cols, d_sums,
                       (long long)min_overlap, gain_mode, (unsigned)strength, d_sharp4, margin, (long long)min_pairs, gate_mode, d_cells, last ? d_image_out : nullptr,
                       last ? d_mask_out : nullptr, last ? d_weight : nullptr, last ? reinterpret_cast<unsigned long long*>(d_counts3) : nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
