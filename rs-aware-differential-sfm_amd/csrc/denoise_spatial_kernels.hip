// denoise_spatial_kernels.hip -- the spatial top-up on MI355X (gfx950, wave64): include/rsdsfm_denoise_spatial.h, defined by
// tests/denoise_spatial_spec_numpy.py and reproduced bit for bit.  Integer arithmetic only; every value goes to memory through ordinary stores and
// atomicAdd.
//   denoise_spatial_kernel<CH, S>  on the 16 x 64 tile of image_tile_device.hpp (the plane reads, the output group and the counters are described
//                               there).
//                               Early exit (uniform over the workgroup): the mask and weight dwords first; where no pixel of the workgroup is set
//                                 and below the target (__syncthreads_or) the image group is copied under the mask (zeros where unset), the
//                                 support is n, and no LDS is filled: a frame the temporal stage fully supported costs a copy.
//                               LDS image: one dword per pixel, the colour bytes in bytes 0 .. 2 and 1 in byte 3 where the pixel is set and inside
//                                 the frame, else 0; halo S + 1 (the candidates' patches); 16 + 2 (S + 1) rows of kStride dwords, the tile's
//                                 pixel (y, x) at [y + S + 1][x + S + 2]: the column in front makes a thread's row window [4 g + 2 .. 4 g + 5 + 2 S]
//                                 start on 8 bytes, so a candidate row is S + 2 ds_read_b64 and serves all 2 S + 1 horizontal displacements.
//                                 kStride = 70 / 74 / 74 (S = 1 / 2 / 3), the smallest stride = 2 mod 4 that holds the 67 + 2 S columns: for
//                                 a 64-bit read the bank is (addr / 4) mod 64 and a wave is served as lanes 0 - 31 and 32 - 63, i.e. two rows
//                                 of 16 threads.  The 16 threads of a row take the bank pairs {4 g + 2 k, 4 g + 2 k + 1}; the next row lies
//                                 kStride = 2 mod 4 dwords on, on the pairs between them -- 32 distinct pairs, no conflict.  (A stride = 0 mod 4,
//                                 68 or 72, would put the second row on the first row's banks.)  The halo is filled byte by byte, mask first.
//                               Per displacement d (all (2 S + 1)^2 - 1; d and -d are not shared): every thread forms
//                                 (both set << 16) | sum_c |I(p) - I(p + d)| of its own four pixels -- one v_sad_u8 of two packed dwords each, the
//                                 validity bytes cancel -- from its registers and the row window, threads 0 .. 163 the halo of 1 from LDS, into
//                                 a second plane of the toolkit's 18 x 66 layout; behind one barrier tile_sum3x3 gives D in the low half and
//                                 the count in the high half (9 * 765 < 2^13), w = 16 - min(16, 16 D / (h CH count)), Sw += w, s_c += w I_c(q).
//                                 The second plane is double-buffered, so a displacement costs one barrier.  The rows of the search are a
//                                 loop, the columns unrolled: the row window is indexed by constants and stays in registers (2 S + 4 dwords; not
//                                 the (3 + 2 S) x (6 + 2 S) window).
//                               Top-up: three 32-bit integer divisions by 2 W per pixel that is smoothed, one more where the support plane is
//                                 asked for; a kept pixel's bytes are copied.
//                               LDS: 5 600 / 6 512 / 7 104 B of image (S = 1 / 2 / 3) plus 9 504 B of the two difference planes.
#include "denoise.hpp"
#include "denoise_spatial_device.hpp"
#include "image_tile_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  out and support (may be NULL) are written whole; counts[0 .. 2] (may be NULL) += [unset,
// kept, smoothed].  weight == NULL: n = 16 where the mask is set
template <int CH, int S>
__global__ __launch_bounds__(kBP) void denoise_spatial_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask,
                                                             const unsigned char* __restrict__ weight, int rows, int cols, unsigned strength, unsigned target,
                                                             unsigned char* __restrict__ out, unsigned char* __restrict__ support,
                                                             unsigned long long* __restrict__ counts) {
#define RSDSFM_SPATIAL_HN_SETUP const unsigned hn = strength * (unsigned)CH;
#define RSDSFM_SPATIAL_HN(j) hn
#include "denoise_spatial_body.hpp"
}

// ---------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------
int denoise_spatial_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, const unsigned char* d_weight, int channels, int rows, int cols, int strength,
                           int target, int search, unsigned char* d_image_out, unsigned char* d_support, int64_t* d_counts3) {
    if (d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, int, int, unsigned, unsigned, unsigned char*, unsigned char*, unsigned long long*);
    static const Kernel kernels[2][3] = {{denoise_spatial_kernel<1, 1>, denoise_spatial_kernel<1, 2>, denoise_spatial_kernel<1, 3>},
                                         {denoise_spatial_kernel<3, 1>, denoise_spatial_kernel<3, 2>, denoise_spatial_kernel<3, 3>}};
    hipLaunchKernelGGL(kernels[channels == 3][search - 1], tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_image, d_mask, d_weight, rows, cols, (unsigned)strength,
                       (unsigned)target, d_image_out, d_support, reinterpret_cast<unsigned long long*>(d_counts3));
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
