// denoise_kernels.hip -- the temporal denoise's accumulate on MI355X (gfx950, wave64): include/rsdsfm_denoise.h, defined by
// tests/denoise_spec_numpy.py and reproduced bit for bit.  Integer arithmetic only; every value goes to memory through ordinary stores and atomicAdd.
//   denoise_accumulate_kernel<CH, FIRST, LAST>  on the 16 x 64 tile of image_tile_device.hpp (the plane reads, the LDS layout and its bank argument,
//                               the cells, the output group and the counters are described there).
//                               Stage 1: the two mask dwords first; R's CH dwords only where some pixel has both masks set (FIRST: where mR
//                                 has a byte set), L's only where some pixel has both; per pixel k_c = min(255, (G_c L_c + 32768) >> 16),
//                                 e = sum_c |R_c - k_c| and the packed dword (v << 16) | e goes to LDS, 0 for a pixel outside the frame.  The
//                                 halo byte by byte, masks first.  Each |R - k| is formed once per workgroup (the halo: once more by the
//                                 neighbouring workgroup).
//                               Stage 2: the sum of the 3 x 3 packed dwords is D in the low half (<= 9 * 765 = 6 885) and the count in the high
//                                 half; w = 16 - min(16, 16 D / (h CH count)) where v, else 0.  A mid step (neither FIRST nor LAST) whose four
//                                 weights are 0 neither reads nor writes its cells.  FIRST: the cells are not read.  LAST: the cells are not
//                                 written; out_c = (2 s_c + n) / (2 n) and mask 1 where n > 0, else 0 / 0, the weight plane n: every byte of
//                                 the outputs is written, no preset.
//                               A mid step of a BGR frame moves 3 + 1 + 3 + 1 + 8 + 8 = 24 B per pixel where both masks are set, plus the halo's
//                                 164 / 1024 of the first 8.
//                               Every workgroup computes the CH gains itself from the 8-word record (seam_gain, threads 0 .. CH - 1, through
//                               LDS): no host wait behind the sums kernel.  The three counters [unset, own only, averaged] only in LAST and
//                               only when a counter pointer was passed.
#include <algorithm>

#include "denoise.hpp"
#include "denoise_device.hpp"
#include "image_tile_device.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  Not LAST: cells += the layer's weighted bytes (FIRST: cells = 16 x the reference, then the
// layer).  LAST: out, mask_out and weight (may be NULL) are written whole; counts[0 .. 2] += [unset, own only, averaged].  layer == lmask ==
// NULL: no layer (FIRST and LAST)
template <int CH, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBP) void denoise_accumulate_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                                const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                                const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode, unsigned strength,
                                                                unsigned short* __restrict__ cells, unsigned char* __restrict__ out,
                                                                unsigned char* __restrict__ mask_out, unsigned char* __restrict__ weight,
                                                                unsigned long long* __restrict__ counts) {
    denoise_accumulate_body<CH, FIRST, LAST>(ref, rmask, layer, lmask, rows, cols, sums, min_overlap, gain_mode, strength, cells, out, mask_out, weight, counts);
}

// ---------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------
int denoise_accumulate_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                              int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int strength, uint16_t* d_cells, bool first,
                              bool last, unsigned char* d_image_out, unsigned char* d_mask_out, unsigned char* d_weight, int64_t* d_counts3) {
    if (last && d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, int, int, const unsigned long long*, long long, int,
                            unsigned, unsigned short*, unsigned char*, unsigned char*, unsigned char*, unsigned long long*);
    static const Kernel kernels[2][2][2] = {
        {{denoise_accumulate_kernel<1, false, false>, denoise_accumulate_kernel<1, false, true>},
         {denoise_accumulate_kernel<1, true, false>, denoise_accumulate_kernel<1, true, true>}},
        {{denoise_accumulate_kernel<3, false, false>, denoise_accumulate_kernel<3, false, true>},
         {denoise_accumulate_kernel<3, true, false>, denoise_accumulate_kernel<3, true, true>}}};
    // the outputs are passed only to the instances that write them
    hipLaunchKernelGGL(kernels[channels == 3][first][last], tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_ref, d_rmask, d_layer, d_lmask, rows, cols, d_sums,
                       (long long)min_overlap, gain_mode, (unsigned)strength, d_cells, last ? d_image_out : nullptr, last ? d_mask_out : nullptr,
                       last ? d_weight : nullptr, last ? reinterpret_cast<unsigned long long*>(d_counts3) : nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
