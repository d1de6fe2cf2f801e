// denoise_spatial_device.hpp -- what the two kernels of the spatial top-up share beside their body (denoise_spatial_body.hpp, an included text):
// the LDS image's geometry and the packed pair entry.  denoise_spatial_kernel (denoise_spatial_kernels.hip) takes the strength as an argument,
// denoise_spatial_auto_kernel (noise_kernels.hip) forms it from a noise record on the device.
#pragma once

#include "denoise.hpp"
#include "image_tile_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

template <int S>
struct SpatialLds {
    static constexpr int kHalo = S + 1;
    static constexpr int kRows = kTileRows + 2 * kHalo;
    static constexpr int kCols = kTileCols + 2 * kHalo;               // pixels of a row; column 0 of the LDS row is the alignment column
    static constexpr int kStride = ((kCols + 2) / 4) * 4 + 2;         // the smallest stride = 2 (mod 4) >= kCols + 1
    static constexpr int kWords = kRows * kStride;
    static constexpr int kBand = 2 * kHalo * kCols;                   // the halo's rows above and below
    static constexpr int kHaloPixels = kRows * kCols - kTileRows * kTileCols;
    static_assert(kStride % 4 == 2 && kStride >= kCols + 1 && kStride - 4 < kCols + 1, "see the bank note above");
};

constexpr unsigned kSetBit = 0x01000000u;

// (both set << 16) | sum over the colour bytes of |a - b|; the two validity bytes are equal where it counts
__device__ __forceinline__ unsigned pair_entry(unsigned a, unsigned b) { return (a & b & kSetBit) ? (0x10000u | __builtin_amdgcn_sad_u8(a, b, 0u)) : 0u; }

}  // namespace rsdsfm
