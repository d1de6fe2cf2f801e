// denoise_device.hpp -- the temporal denoise's accumulate as a function that two kernels share: denoise_accumulate_kernel (denoise_kernels.hip), which
// takes the strength as an argument, and denoise_accumulate_auto_kernel (noise_kernels.hip), which forms it from a noise record on the device
// (noise_device.hpp).  __device__ __forceinline__, as plate_device.hpp serves the median and the medoid: either kernel is the code it would be
// with its own copy.  Its statements are denoise_accumulate_body.hpp's, the one text that denoise_accumulate_curve_kernel
// (noise_curve_kernels.hip) includes too, with a strength per pixel.
#pragma once

#include "denoise.hpp"
#include "image_tile_device.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

template <int CH, bool FIRST, bool LAST>
__device__ __forceinline__ void denoise_accumulate_body(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                        const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                        const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode, unsigned strength,
                                                        unsigned short* __restrict__ cells, unsigned char* __restrict__ out, unsigned char* __restrict__ mask_out,
                                                        unsigned char* __restrict__ weight, unsigned long long* __restrict__ counts) {
#define RSDSFM_ACCUMULATE_TABLE
#define RSDSFM_ACCUMULATE_STRENGTH(j) strength
#include "denoise_accumulate_body.hpp"
}

}  // namespace rsdsfm
