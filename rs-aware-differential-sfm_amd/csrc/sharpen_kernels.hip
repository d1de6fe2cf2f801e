// sharpen_kernels.hip -- the sharpen stage's kernel (include/rsdsfm_sharpen.h; tests/sharpen_spec_numpy.py is the definition; DESIGN section 12,
// "Sharpen"): a noise-gated unsharp mask on the image stages' 16 x 64 tile.
//   sharpen_kernel<CH, CURVE>   four instances.  A thread owns 4 consecutive pixels.  The tile and a halo of 2 are staged ONCE in LDS, a packed
//                               dword per pixel (SharpenLds, sharpen.hpp: 20 x 70 dwords, 5.6 KB); unset pixels and pixels outside the frame are
//                               0, so the sums need no mask.  Per thread five rows of four 8-byte LDS reads (20 reads, 10 dwords per pixel) give
//                               the 5 x 8 window.  A dword splits into two dwords of 16-bit fields, (c0, c2) and (c1, set bit): the binomial sums
//                               S_c <= 255 * 256 and K <= 256 fit their fields, so ONE multiply-add per dword and tap serves two fields --
//                               vertical [1, 4, 6, 4, 1] into eight column sums, then horizontal per pixel.  The 3 x 3 minimum and maximum run on
//                               the same fields (v_pk_min_u16 / v_pk_max_u16), unset pixels entering the minimum as 255 and the maximum as 0.
//                               The one division per channel, by 16 K, is a float reciprocal corrected by its remainder (div_u24: exact).
//                               CURVE: the 256-entry strength table in LDS, formed per workgroup by noise_curve_entry (noise_curve.hpp), the
//                               text the curve top-up and the host's rsdsfm_noise_curve_strengths run.
//                               A workgroup without a set pixel of its own, or amount_q4 = 0, stages nothing: it copies under the mask.
//                               Stores through store_group, counters through block_counts_add<4>.
#include <hip/hip_runtime.h>

#include "sharpen.hpp"

namespace rsdsfm {

namespace {

static_assert(kBP == 256, "one thread per entry of the strength table");
constexpr unsigned kLoFields = 0x00ff00ffu;

}  // namespace

template <int CH, bool CURVE>
__global__ __launch_bounds__(kBP) void sharpen_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask, int rows, int cols, unsigned amount,
                                                      unsigned coring, unsigned overshoot, unsigned strength, const unsigned long long* __restrict__ curve36, unsigned scale,
                                                      long long min_samples, long long band_min_samples, unsigned char* __restrict__ out,
                                                      unsigned long long* __restrict__ counts) {
    using L = SharpenLds;
    __shared__ __attribute__((aligned(16))) unsigned s_img[L::kWords];
    __shared__ unsigned char s_lut[CURVE ? 256 : 4];
    const TileThread t = tile_thread(rows, cols);
    const int nin = t.nin;
    const int64_t p0 = t.p0, npix = (int64_t)rows * cols;

    unsigned mv = 0u, iw[CH];
#pragma unroll
    for (int d = 0; d < CH; ++d) iw[d] = 0u;
    if (nin) {
        unsigned w1[1];
        load_bytes<1>(mask, p0, npix, w1);
        mv = bytes_set(w1[0]) & first_ones(nin);
        if (mv) load_bytes<CH>(image, (int64_t)CH * p0, (int64_t)CH * npix, iw);  // image bytes under an empty mask are not read
    }
    unsigned pk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool vj = ((mv >> (8 * j)) & 1u) != 0u;
        unsigned b = kSetBit;
#pragma unroll
        for (int c = 0; c < CH; ++c) b |= byte_of(iw, CH * j + c) << (8 * c);
        pk[j] = vj ? b : 0u;
    }
    // nothing to sharpen in this tile: the output is the input under the mask (uniform)
    const bool active = amount != 0u && __syncthreads_or(mv != 0u ? 1 : 0) != 0;

    unsigned ow[CH], n4[4] = {0u, 0u, 0u, 0u};  // [unset, kept, sharpened, limited]; at most 4 per thread
#pragma unroll
    for (int d = 0; d < CH; ++d) ow[d] = 0u;

    if (active) {
        if constexpr (CURVE) s_lut[t.tid] = (unsigned char)noise_curve_entry(curve36, scale, strength, min_samples, band_min_samples, t.tid);
        unsigned* own = s_img + (t.ty + L::kHalo) * L::kStride + 4 * t.g + L::kHalo;
#pragma unroll
        for (int j = 0; j < 4; ++j) own[j] = pk[j];
        sharpen_load_halo<CH>(s_img, t, image, mask, rows, cols);
        __syncthreads();

        // the 5 x 8 window: rows ty .. ty + 4 of the LDS image, pixels 4 g - 2 .. 4 g + 5
        unsigned colE[8], colO[8], minE[6], minO[6], maxE[6], maxO[6];
        const unsigned* row0 = s_img + t.ty * L::kStride + 4 * t.g;
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const unsigned kv = r == 0 || r == 4 ? 1u : r == 2 ? 6u : 4u;
            unsigned win[8];
            const Lds8* q8 = static_cast<const Lds8*>(__builtin_assume_aligned(row0 + r * L::kStride, 8));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const Lds8 v = q8[k];
                win[2 * k] = v[0];
                win[2 * k + 1] = v[1];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const unsigned e = win[i] & kLoFields, o = (win[i] >> 8) & kLoFields;  // (c0, c2), (c1, set)
                colE[i] = r == 0 ? e : colE[i] + kv * e;
                colO[i] = r == 0 ? o : colO[i] + kv * o;
                if (r >= 1 && r <= 3 && i >= 1 && i <= 6) {
                    const bool set = (win[i] & kSetBit) != 0u;
                    const unsigned le = set ? e : kLoFields, lo = set ? o : kLoFields;  // unset: 255 for the minimum; e = o = 0 already for the maximum
                    minE[i - 1] = r == 1 ? le : pk_min_u16(minE[i - 1], le);
                    minO[i - 1] = r == 1 ? lo : pk_min_u16(minO[i - 1], lo);
                    maxE[i - 1] = r == 1 ? e : pk_max_u16(maxE[i - 1], e);
                    maxO[i - 1] = r == 1 ? o : pk_max_u16(maxO[i - 1], o);
                }
            }
        }

#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool vj = (pk[j] & kSetBit) != 0u;
            const unsigned SE = colE[j] + 4u * colE[j + 1] + 6u * colE[j + 2] + 4u * colE[j + 3] + colE[j + 4];
            const unsigned SO = colO[j] + 4u * colO[j + 1] + 6u * colO[j + 2] + 4u * colO[j + 3] + colO[j + 4];
            const unsigned loE = pk_min_u16(pk_min_u16(minE[j], minE[j + 1]), minE[j + 2]), loO = pk_min_u16(pk_min_u16(minO[j], minO[j + 1]), minO[j + 2]);
            const unsigned hiE = pk_max_u16(pk_max_u16(maxE[j], maxE[j + 1]), maxE[j + 2]), hiO = pk_max_u16(pk_max_u16(maxO[j], maxO[j + 1]), maxO[j + 2]);
            const unsigned K = vj ? SO >> 16 : 1u;  // >= 36 where set
            unsigned h = strength;
            if constexpr (CURVE) h = s_lut[sharpen_level<CH>(pk[j])];
            unsigned T = (coring * h + 8u) >> 4;
            T = T > 255u ? 255u : T;  // |d| < 255 K: from 255 on nothing passes
            const unsigned TK = T * K, den = 16u * K;
            bool changed = false, limited = false;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const unsigned I = (pk[j] >> (8 * c)) & 0xffu;
                const unsigned S = c == 0 ? SE & 0xffffu : c == 1 ? SO & 0xffffu : SE >> 16;
                const int lo = (int)(c == 0 ? loE & 0xffffu : c == 1 ? loO & 0xffffu : loE >> 16);
                const int hi = (int)(c == 0 ? hiE & 0xffffu : c == 1 ? hiO & 0xffffu : hiE >> 16);
                const int d = (int)(K * I) - (int)S;
                const unsigned a = (unsigned)(d < 0 ? -d : d);
                const unsigned e = a > TK ? a - TK : 0u;
                const int r = (int)div_u24(amount * e + 8u * K, den);  // = (2 amount e + 16 K) / (32 K)
                const int o = (int)I + (d < 0 ? -r : r);
                const int lim_lo = lo - (int)overshoot < 0 ? 0 : lo - (int)overshoot, lim_hi = hi + (int)overshoot > 255 ? 255 : hi + (int)overshoot;
                const int res = o < lim_lo ? lim_lo : o > lim_hi ? lim_hi : o;
                const unsigned val = vj ? (unsigned)res : 0u;
                changed = changed || (vj && val != I);
                limited = limited || (vj && res != o);
                ow[(CH * j + c) >> 2] |= val << (8 * ((CH * j + c) & 3));
            }
            if (j < nin) {
                n4[0] += vj ? 0u : 1u;
                n4[1] += vj && !changed ? 1u : 0u;
                n4[2] += changed && !limited ? 1u : 0u;
                n4[3] += changed && limited ? 1u : 0u;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool vj = (pk[j] & kSetBit) != 0u;
#pragma unroll
            for (int c = 0; c < CH; ++c) ow[(CH * j + c) >> 2] |= ((pk[j] >> (8 * c)) & 0xffu) << (8 * ((CH * j + c) & 3));
            if (j < nin) {
                n4[0] += vj ? 0u : 1u;
                n4[1] += vj ? 1u : 0u;
            }
        }
    }
    if (nin) {
        unsigned char* const planes[1] = {nullptr};
        const unsigned words[1] = {0u};
        store_group<CH>(out, ow, planes, words, p0, nin);
    }
    block_counts_add<4>(n4, counts);
}

// ---------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------
int sharpen_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, int channels, int rows, int cols, int amount_q4, int coring_q4, int overshoot,
                   int strength, const unsigned long long* d_curve36, int scale, int64_t min_samples, int64_t band_min_samples, unsigned char* d_image_out,
                   int64_t* d_counts4) {
    if (d_counts4) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts4, 0, kSharpenCounters * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const unsigned char*, const unsigned char*, int, int, unsigned, unsigned, unsigned, unsigned, const unsigned long long*, unsigned, long long,
                            long long, unsigned char*, unsigned long long*);
    static const Kernel kernels[2][2] = {{sharpen_kernel<1, false>, sharpen_kernel<1, true>}, {sharpen_kernel<3, false>, sharpen_kernel<3, true>}};
    hipLaunchKernelGGL(kernels[channels == 3][d_curve36 != nullptr], tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_image, d_mask, rows, cols, (unsigned)amount_q4,
                       (unsigned)coring_q4, (unsigned)overshoot, (unsigned)strength, d_curve36, (unsigned)scale, (long long)min_samples, (long long)band_min_samples,
                       d_image_out, reinterpret_cast<unsigned long long*>(d_counts4));
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
