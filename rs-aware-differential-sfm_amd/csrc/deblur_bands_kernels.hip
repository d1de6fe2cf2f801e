// deblur_bands_kernels.hip -- the sharpness transfer per scanline band on MI355X (gfx950, wave64): include/rsdsfm_deblur.h ("per scanline
// band"), defined by tests/deblur_bands_spec_numpy.py and reproduced bit for bit.  A rolling-shutter frame's blur varies down the frame, so the
// frame is cut into bands of band_rows = H rows (a multiple of the tile's 16, so that a tile lies in one band), every band has its own record
// and its own tau, and a row's tau is interpolated between the two band centres about it.  Both kernels are the bodies of deblur_sharpness_body.hpp and
// deblur_device.hpp, the ones deblur_kernels.hip builds with one record: the tile, its LDS layout and bank argument (image_tile_device.hpp), the plane reads, the
// cells, the outputs and the counters are those.  Integer arithmetic only; every value goes to memory through ordinary stores and atomicAdd.
//   deblur_band_sharpness_kernel<CH>   the sharpness body with the workgroup's three sums added to record (16 blockIdx.y) / H.  A pair belongs
//                               to its left or upper pixel and the body counts it in that pixel's tile, so a vertical pair across a band
//                               border lands in the upper band and the records summed are the whole-frame record.  The same three 64-bit
//                               atomics per workgroup: exact and independent of scheduling.
//   deblur_band_accumulate_kernel<CH, FIRST, LAST>  the accumulate body with BANDS: threads CH .. CH + 2 compute tau of the bands b - 1, b, b + 1
//                               of the tile's band b (one 64-bit division each, beside the gains; the indices clamped to [0, NB - 1], so no
//                               read leaves the NB records), through LDS; threads 0 .. 15 then compute the tile's 16 row taus
//                               (deblur_row_tau_of, one 32-bit division each) and share them through LDS; a thread takes its row's.  A launch
//                               that is neither FIRST nor LAST returns after the records when all three taus are 0: no row of the tile can get
//                               a tau then, and a blurred band of a sharp neighbour costs no image bytes.
#include "deblur.hpp"
#include "deblur_device.hpp"
#include "image_tile_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  records: ceil(rows / band_rows) records, zeroed by the caller; band_rows % 16 == 0
template <int CH>
__global__ __launch_bounds__(kBP) void deblur_band_sharpness_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                                   const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows,
                                                                   int cols, const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode,
                                                                   int band_rows, unsigned long long* __restrict__ records) {
    unsigned long long* const T = records + 4 * (((int)blockIdx.y * kTileRows) / band_rows);  // blockIdx.y * 16 < rows, so the band is < ceil(rows / band_rows)
#include "deblur_sharpness_body.hpp"
}

template <int CH, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBP) void deblur_band_accumulate_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                                    const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows,
                                                                    int cols, const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode,
                                                                    unsigned strength, const unsigned long long* __restrict__ records, int band_rows, int nbands,
                                                                    int margin, long long min_pairs, int gate_mode, unsigned short* __restrict__ cells,
                                                                    unsigned char* __restrict__ out, unsigned char* __restrict__ mask_out,
                                                                    unsigned char* __restrict__ weight, unsigned long long* __restrict__ counts) {
    deblur_accumulate_body<CH, FIRST, LAST, true>(ref, rmask, layer, lmask, rows, cols, sums, min_overlap, gain_mode, strength, records, band_rows, nbands, margin,
                                                  min_pairs, gate_mode, cells, out, mask_out, weight, counts);
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int deblur_band_sharpness_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                                 int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int band_rows, unsigned long long* d_records) {
    RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_records, 0, (size_t)deblur_bands_of(rows, band_rows) * 4 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(channels == 3 ? deblur_band_sharpness_kernel<3> : deblur_band_sharpness_kernel<1>, tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_ref, d_rmask,
                       d_layer, d_lmask, rows, cols, d_sums, (long long)min_overlap, gain_mode, band_rows, d_records);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int deblur_band_accumulate_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                                  int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int strength,
                                  const unsigned long long* d_records, int band_rows, int margin, int64_t min_pairs, int gate_mode, uint16_t* d_cells, bool first, bool last,
                                  unsigned char* d_image_out, unsigned char* d_mask_out, unsigned char* d_weight, int64_t* d_counts3) {
    if (last && d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, int, int, const unsigned long long*, long long, int,
                            unsigned, const unsigned long long*, int, int, int, long long, int, unsigned short*, unsigned char*, unsigned char*, unsigned char*,
                            unsigned long long*);
    static const Kernel kernels[2][2][2] = {
        {{deblur_band_accumulate_kernel<1, false, false>, deblur_band_accumulate_kernel<1, false, true>},
         {deblur_band_accumulate_kernel<1, true, false>, deblur_band_accumulate_kernel<1, true, true>}},
        {{deblur_band_accumulate_kernel<3, false, false>, deblur_band_accumulate_kernel<3, false, true>},
         {deblur_band_accumulate_kernel<3, true, false>, deblur_band_accumulate_kernel<3, true, true>}}};
    // the outputs are passed only to the instances that write them
    hipLaunchKernelGGL(kernels[channels == 3][first][last], tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_ref, d_rmask, d_layer, d_lmask, rows, cols, d_sums,
                       (long long)min_overlap, gain_mode, (unsigned)strength, d_records, band_rows, deblur_bands_of(rows, band_rows), margin, (long long)min_pairs, gate_mode,
                       d_cells, last ? d_image_out : nullptr, last ? d_mask_out : nullptr, last ? d_weight : nullptr,
                       last ? reinterpret_cast<unsigned long long*>(d_counts3) : nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
