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
#include "image_tile_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace {

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

}  // namespace

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  out and support (may be NULL) are written whole; counts[0 .. 2] (may be NULL) += [unset,
// kept, smoothed].  weight == NULL: n = 16 where the mask is set
template <int CH, int S>
__global__ __launch_bounds__(kBP) void denoise_spatial_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask,
                                                             const unsigned char* __restrict__ weight, int rows, int cols, unsigned strength, unsigned target,
                                                             unsigned char* __restrict__ out, unsigned char* __restrict__ support,
                                                             unsigned long long* __restrict__ counts) {
    using L = SpatialLds<S>;
    __shared__ __attribute__((aligned(16))) unsigned s_img[L::kWords];
    __shared__ __attribute__((aligned(16))) unsigned s_e[2][kTileLdsWords];
    const TileThread t = tile_thread(rows, cols);
    const int nin = t.nin;
    const int64_t p0 = t.p0, npix = (int64_t)rows * cols;

    unsigned mv = 0u, nw = 0u, iw[CH];
#pragma unroll
    for (int d = 0; d < CH; ++d) iw[d] = 0u;
    if (nin) {  // the mask and weight dwords first
        unsigned w1[1];
        load_bytes<1>(mask, p0, npix, w1);
        mv = bytes_set(w1[0]) & first_ones(nin);
        if (mv) {  // neither weights nor image bytes under an empty mask are read
            nw = kDenoiseW * 0x01010101u;
            if (weight) {
                load_bytes<1>(weight, p0, npix, w1);
                nw = w1[0];
            }
            load_bytes<CH>(image, (int64_t)CH * p0, (int64_t)CH * npix, iw);
        }
    }
    unsigned pk[4], nj[4];
    bool need = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool vj = ((mv >> (8 * j)) & 1u) != 0u;
        nj[j] = (nw >> (8 * j)) & 0xffu;
        need = need || (vj && nj[j] < target);
        unsigned b = kSetBit;
#pragma unroll
        for (int c = 0; c < CH; ++c) b |= byte_of(iw, CH * j + c) << (8 * c);
        pk[j] = vj ? b : 0u;
    }
    const bool any_need = __syncthreads_or(need ? 1 : 0) != 0;  // (uniform)

    unsigned sw[4] = {0u, 0u, 0u, 0u}, sc[4][CH];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < CH; ++c) sc[j][c] = 0u;

    if (any_need) {
        // the LDS image: the thread's own four pixels, then the halo of S + 1
        unsigned* own = s_img + (t.ty + L::kHalo) * L::kStride + 4 * t.g + L::kHalo + 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) own[j] = pk[j];
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
            s_img[r * L::kStride + cc + 1] = b;
        }
        __syncthreads();

        const unsigned* row0 = s_img + (t.ty + L::kHalo) * L::kStride + 4 * t.g + 2;  // the thread's row window at dy = 0: pixel 4 g - S of the tile
        const int own_e = (t.ty + 1) * kTileLdsStride + 4 * t.g + 1;
        const bool is_halo = t.tid < kTileHalo;
        const TileHalo h = tile_halo(t);
        const int halo_e = h.ly * kTileLdsStride + h.lx, halo_i = (h.ly + S) * L::kStride + h.lx + S + 1;
        const unsigned hn = strength * (unsigned)CH;
        int buf = 0;
#pragma unroll 1
        for (int dy = -S; dy <= S; ++dy) {
            unsigned win[2 * S + 4];
            const Lds8* q8 = static_cast<const Lds8*>(__builtin_assume_aligned(row0 + dy * L::kStride, 8));
#pragma unroll
            for (int k = 0; k < S + 2; ++k) {
                const Lds8 v = q8[k];
                win[2 * k] = v[0];
                win[2 * k + 1] = v[1];
            }
#pragma unroll
            for (int dx = -S; dx <= S; ++dx) {
                if (dx == 0 && dy == 0) continue;  // (uniform)
                unsigned* e = s_e[buf];
                unsigned ent[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ent[j] = pair_entry(pk[j], win[j + dx + S]);
                    e[own_e + j] = ent[j];
                }
                if (is_halo) e[halo_e] = pair_entry(s_img[halo_i], s_img[halo_i + dy * L::kStride + dx]);
                __syncthreads();  // the other plane was last read in front of this barrier: one barrier per displacement
                if (need) {
                    unsigned col[6];
                    tile_sum3x3(e, t.ty, t.g, col);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (ent[j]) {  // p and q both set: the patch counts at least o = 0
                            const unsigned s = col[j] + col[j + 1] + col[j + 2];
                            const unsigned qd = (kDenoiseW * (s & 0xffffu)) / (hn * (s >> 16));
                            const unsigned w = kDenoiseW - (qd > kDenoiseW ? kDenoiseW : qd);
                            const unsigned q = win[j + dx + S];
                            sw[j] += w;
#pragma unroll
                            for (int c = 0; c < CH; ++c) sc[j][c] += w * ((q >> (8 * c)) & 0xffu);
                        }
                    }
                }
                buf ^= 1;
            }
        }
    }

    // the top-up; without any_need every set pixel is kept
    unsigned ow[CH], sup = 0u, n3[3] = {0u, 0u, 0u};  // [unset, kept, smoothed]; at most 4 per thread
#pragma unroll
    for (int d = 0; d < CH; ++d) ow[d] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool vj = (pk[j] & kSetBit) != 0u;
        const unsigned n = nj[j], delta = target > n ? target - n : 0u;
        const unsigned B = sw[j] > 8u * kDenoiseW ? sw[j] : 8u * kDenoiseW;
        const unsigned add = delta * sw[j], Wt = n * B + add;
        const bool smooth = vj && add != 0u;  // then Wt > 0
        unsigned s8 = vj ? n : 0u;            // a kept pixel's support: (2 n B + B) / (2 B) = n
        if (smooth && support) {              // (support: uniform)
            const unsigned sv = (2u * Wt + B) / (2u * B);
            s8 = sv > 255u ? 255u : sv;
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const unsigned I = (pk[j] >> (8 * c)) & 0xffu;  // 0 where unset
            const unsigned val = smooth ? (2u * (n * B * I + delta * sc[j][c]) + Wt) / (2u * Wt) : I;  // round half up; < 2^31
            ow[(CH * j + c) >> 2] |= val << (8 * ((CH * j + c) & 3));
        }
        sup |= s8 << (8 * j);
        if (j < nin) {
            n3[0] += vj ? 0u : 1u;
            n3[1] += vj && !smooth ? 1u : 0u;
            n3[2] += smooth ? 1u : 0u;
        }
    }
    if (nin) {
        unsigned char* const planes[1] = {support};
        const unsigned words[1] = {sup};
        store_group<CH>(out, ow, planes, words, p0, nin);
    }
    block_counts_add<3>(n3, counts);
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
