// sharpen.hpp -- the sharpen stage (include/rsdsfm_sharpen.h): what sharpen_kernels.hip and sharpen_host.hip share, and the few device
// blocks the tile toolkit (image_tile_device.hpp) lacks for a halo of 2.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_sharpen.h"
#include "noise_curve.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

constexpr int kSharpenAmountDefault = RSDSFM_SHARPEN_AMOUNT_DEFAULT, kSharpenAmountMax = RSDSFM_SHARPEN_AMOUNT_MAX;
constexpr int kSharpenCoringDefault = RSDSFM_SHARPEN_CORING_DEFAULT, kSharpenCoringMax = RSDSFM_SHARPEN_CORING_MAX;
constexpr int kSharpenOvershootDefault = RSDSFM_SHARPEN_OVERSHOOT_DEFAULT, kSharpenOvershootMax = RSDSFM_SHARPEN_OVERSHOOT_MAX;
constexpr int kSharpenCounters = 4;  // [unset, kept, sharpened, limited]

// on c->stream (arguments checked and defaults resolved by the caller): the counters zeroed by a memset, then the one launch.  d_curve36 NULL:
// the fixed strength (sharpen_kernel<CH, false>); else `strength` is the fallback (sharpen_kernel<CH, true>)
int sharpen_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, int channels, int rows, int cols, int amount_q4, int coring_q4, int overshoot,
                   int strength, const unsigned long long* d_curve36, int scale, int64_t min_samples, int64_t band_min_samples, unsigned char* d_image_out,
                   int64_t* d_counts4);

}  // namespace rsdsfm

#if defined(__HIPCC__)
#include "denoise_spatial_device.hpp"
#include "image_tile_device.hpp"

namespace rsdsfm {

// The LDS image: one packed dword per pixel (colour in bytes 0 .. 2, kSetBit above them; 0 where unset or outside the frame), the tile and a
// halo of 2: 20 rows x 68 pixels at the top-up's row stride for the same halo, 70 dwords (SpatialLds<1>: = 2 mod 4).  The tile's pixel (y, x)
// lies at [y + 2][x + 2] -- NOT behind the top-up's alignment column: a thread's 5 x 8 window starts at pixel 4 g - 2, dword 4 g of its row,
// which is 8-byte aligned as it stands (70 and 4 g are even), so each row is four 8-byte reads.  Banks, by the rule at the top of
// image_tile_device.hpp: the 16 threads of a row read bank pairs {4 g + 2 k, 4 g + 2 k + 1}, the next row's 16 threads lie 70 = 6 (mod 64)
// banks on, pairs that start at 2 (mod 4): the 32 lanes of a group take 32 distinct pairs -- no conflict, for every one of the 20 reads.
struct SharpenLds {
    static constexpr int kHalo = 2;
    static constexpr int kRows = kTileRows + 2 * kHalo;  // 20
    static constexpr int kCols = kTileCols + 2 * kHalo;  // 68
    static constexpr int kStride = SpatialLds<1>::kStride;  // 70
    static constexpr int kWords = kRows * kStride;       // 1400 dwords = 5600 B
    static constexpr int kBand = 2 * kHalo * kCols;      // the halo's rows above and below
    static constexpr int kHaloPixels = kRows * kCols - kTileRows * kTileCols;  // 336
    static_assert(SpatialLds<1>::kHalo == kHalo && kStride % 4 == 2 && kStride >= kCols, "the top-up's stride for a halo of 2");
};

// x / 3 for x <= 766 as a multiply-shift (the noise curve's; tests/test_noise_curve_cpu.py proves it exact)
__device__ __forceinline__ unsigned sharpen_third(unsigned x) { return (x * 21846u) >> 16; }

// the level of a packed pixel, as the noise curve's consumers take it: its byte (gray) or (b + g + r + 1) / 3 (BGR)
template <int CH>
__device__ __forceinline__ unsigned sharpen_level(unsigned packed) {
    if constexpr (CH == 1) return packed & 0xffu;
    return sharpen_third((packed & 0xffu) + ((packed >> 8) & 0xffu) + ((packed >> 16) & 0xffu) + 1u);
}

// the halo of 2 about the tile into s_img, the top-up's loader (denoise_spatial_body.hpp) without its alignment column: 336 pixels, at most
// two per thread
template <int CH>
__device__ __forceinline__ void sharpen_load_halo(unsigned* s_img, const TileThread& t, const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask, int rows,
                                                  int cols) {
    using L = SharpenLds;
    for (int i = t.tid; i < L::kHaloPixels; i += kBP) {
        int r, cc;
        if (i < L::kBand) {
            r = i / L::kCols;
            cc = i - r * L::kCols;
            r = r < L::kHalo ? r : r + kTileRows;
        } else {
            const int k = i - L::kBand;
            r = k / (2 * L::kHalo);
            cc = k - r * (2 * L::kHalo);
            r += L::kHalo;
            cc = cc < L::kHalo ? cc : cc + kTileCols;
        }
        const int hy = t.y0 - L::kHalo + r, hx = t.x0 - L::kHalo + cc;
        unsigned b = 0u;
        if (hy >= 0 && hy < rows && hx >= 0 && hx < cols) {
            const int64_t p = (int64_t)hy * cols + hx;
            if (mask[p] != 0) {
                b = kSetBit;
#pragma unroll
                for (int c = 0; c < CH; ++c) b |= (unsigned)image[CH * p + c] << (8 * c);
            }
        }
        s_img[r * L::kStride + cc] = b;
    }
}

// two 16-bit fields per dword
typedef unsigned short Half2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_min_u16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(Half2, a), __builtin_bit_cast(Half2, b)));
}
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(Half2, a), __builtin_bit_cast(Half2, b)));
}

// num / den for num < 2^24 and 1 <= den < 2^24, exact: both are exact floats, the reciprocal's and the product's errors together stay far
// below 1 (the quotient is below 2^14 here), so the estimate is off by at most one, which the remainder corrects
__device__ __forceinline__ unsigned div_u24(unsigned num, unsigned den) {
    unsigned q = (unsigned)((float)num * __builtin_amdgcn_rcpf((float)den));
    const int rem = (int)num - (int)(q * den);
    q = rem < 0 ? q - 1u : rem >= (int)den ? q + 1u : q;
    return q;
}

}  // namespace rsdsfm
#endif
