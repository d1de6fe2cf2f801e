// deblur_device.hpp -- what the sharpness transfer's two translation units share on the device (deblur_kernels.hip: one tau per layer;
// deblur_bands_kernels.hip: a tau per band of rows), the way plate_device.hpp serves the median and the medoid: the packed pair and the
// accumulate body, __device__ __forceinline__, so that a kernel built from them is the code it was when it carried its own copy
// (profiles/deblur_bands_isa.txt); the sharpness kernels' body is deblur_sharpness_body.hpp.  The bodies are described in deblur_kernels.hip's
// header; BANDS is described in deblur_bands_kernels.hip's.
#pragma once

#include "deblur.hpp"
#include "image_tile_device.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace {

constexpr unsigned kSharpV = 1u << 20;

// one pair of packed pixels a (set) and b: counted when b is set too
__device__ __forceinline__ void sharp_pair(unsigned a, unsigned b, unsigned (&n3)[3]) {
    if (b) {
        const int dr = (int)((a >> 10) & 1023u) - (int)((b >> 10) & 1023u);
        const int dl = (int)(a & 1023u) - (int)(b & 1023u);
        n3[0] += 1u;
        n3[1] += (unsigned)(dr * dr);  // <= 765^2 = 585 225; a thread's eight pairs < 2^23
        n3[2] += (unsigned)(dl * dl);
    }
}

// BANDS false: sharp is the layer's one record and tau one number (band_rows and nbands are not read).  BANDS true: sharp is nbands records and
// tau a number per row of the tile
template <int CH, bool FIRST, bool LAST, bool BANDS>
__device__ __forceinline__ void deblur_accumulate_body(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                       const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                       const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode, unsigned strength,
                                                       const unsigned long long* __restrict__ sharp, int band_rows, int nbands, int margin, long long min_pairs,
                                                       int gate_mode, unsigned short* __restrict__ cells, unsigned char* __restrict__ out,
                                                       unsigned char* __restrict__ mask_out, unsigned char* __restrict__ weight, unsigned long long* __restrict__ counts) {
    constexpr int H = CH + 1;     // halfwords per cell
    constexpr int NW = 4 * H / 2; // dwords of a thread's four cells: 8 (BGR) or 4 (gray)
    __shared__ __attribute__((aligned(16))) unsigned s_tile[kTileLdsWords];
    __shared__ unsigned s_gain[CH + 1];  // the gains, then tau
    const TileThread t = tile_thread(rows, cols);
    unsigned tau = 0u;
    [[maybe_unused]] bool band_layer = false;  // (uniform) BANDS: some row of the tile may get a tau
    if (layer != nullptr) {  // (uniform)
        if (t.tid < CH) s_gain[t.tid] = sums ? seam_gain(sums, CH, t.tid, min_overlap, gain_mode) : kGainOne;
        if constexpr (BANDS) {
            __shared__ unsigned s_band[3];         // tau of the band above, of the tile's band and of the band below
            __shared__ unsigned s_row[kTileRows];  // tau of the tile's 16 rows
            const int b = t.y0 / band_rows;        // < nbands: y0 < rows
            if (t.tid >= CH && t.tid < CH + 3) {
                const int k = t.tid - CH, i = b + k - 1;
                s_band[k] = deblur_tau_of(sharp + 4 * (i < 0 ? 0 : i > nbands - 1 ? nbands - 1 : i), margin, min_pairs);  // no read leaves the nbands records
            }
            __syncthreads();
            const unsigned ta = s_band[0], tb = s_band[1], tc = s_band[2];
            band_layer = (ta | tb | tc) != 0u;
            if (!FIRST && !LAST && !band_layer) return;  // (uniform) no row of the tile can get a tau: no image byte is read
            if (t.tid < kTileRows) s_row[t.tid] = deblur_row_tau_of(t.y0 + t.tid, b, band_rows, nbands, ta, tb, tc);
            __syncthreads();
            tau = s_row[t.ty];
        } else {
            if (t.tid == CH) s_gain[CH] = deblur_tau_of(sharp, margin, min_pairs);
            __syncthreads();
            tau = s_gain[CH];
            if (!FIRST && !LAST && tau == 0u) return;  // (uniform) a layer that is no sharper adds nothing: no image byte is read
        }
    }
    const bool has_layer = BANDS ? band_layer : tau != 0u;  // (uniform)
    const int nin = t.nin;
    const int64_t p0 = t.p0, npix = (int64_t)rows * cols;
    const unsigned inside = first_ones(nin);

    unsigned mr = 0u, v = 0u, rw[CH], kk[4][CH], wgt[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < CH; ++d) rw[d] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < CH; ++c) kk[j][c] = 0u;

    if (nin) {  // the mask dwords first
        unsigned w1[1];
        load_bytes<1>(rmask, p0, npix, w1);
        mr = bytes_set(w1[0]) & inside;
        if (has_layer && mr) {
            load_bytes<1>(lmask, p0, npix, w1);
            v = bytes_set(w1[0]) & mr;
        }
        if (FIRST ? mr != 0u : v != 0u) load_bytes<CH>(ref, (int64_t)CH * p0, (int64_t)CH * npix, rw);  // image bytes under an empty mask are not read
    }

    if (has_layer) {
        unsigned G[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) G[c] = s_gain[c];
        // stage 1: the thread's own four pixels
        unsigned ent[4] = {0u, 0u, 0u, 0u};
        if (v) {
            unsigned lw[CH];
            load_bytes<CH>(layer, (int64_t)CH * p0, (int64_t)CH * npix, lw);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned yr = 0u, yl = 0u;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    kk[j][c] = gained(G[c], byte_of(lw, CH * j + c));
                    yr += byte_of(rw, CH * j + c);
                    yl += kk[j][c];
                }
                ent[j] = ((v >> (8 * j)) & 1u) ? (0x10000u | (yr + kDeblurBias - yl)) : 0u;
            }
        }
        unsigned* row = tile_own(s_tile, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) row[j] = ent[j];
        if (t.tid < kTileHalo) {
            const TileHalo h = tile_halo(t);
            unsigned e = 0u;
            if (h.hy >= 0 && h.hy < rows && h.hx >= 0 && h.hx < cols) {
                const int64_t p = (int64_t)h.hy * cols + h.hx;
                if (rmask[p] != 0 && lmask[p] != 0) {
                    e = 0x10000u | kDeblurBias;
#pragma unroll
                    for (int c = 0; c < CH; ++c) e += (unsigned)ref[CH * p + c] - gained(G[c], layer[CH * p + c]);  // the sum stays in [0, 1530]
                }
            }
            s_tile[h.ly * kTileLdsStride + h.lx] = e;
        }
        __syncthreads();
        // stage 2: the 3 x 3 sums of the packed dwords
        if (v) {
            unsigned col[6];
            tile_sum3x3(s_tile, t.ty, t.g, col);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned s = col[j] + col[j + 1] + col[j + 2];
                const unsigned low = s & 0xffffu, cnt = s >> 16, mid = kDeblurBias * cnt;
                if ((v >> (8 * j)) & 1u) {  // the pixel itself counts: cnt >= 1
                    const unsigned D = low > mid ? low - mid : mid - low;
                    const unsigned qd = (kDenoiseW * D) / (strength * (unsigned)CH * cnt);
                    const unsigned w = gate_mode == 1 ? kDenoiseW : kDenoiseW - (qd > kDenoiseW ? kDenoiseW : qd);
                    wgt[j] = (w * tau + 8u) >> 4;  // <= 32
                }
            }
        }
    }

    unsigned n3[3] = {0u, 0u, 0u};  // [unset, own only, transferred]; at most 4 per thread
    const bool any_w = (wgt[0] | wgt[1] | wgt[2] | wgt[3]) != 0u;
    if (nin && (FIRST || LAST || any_w)) {  // a mid step that adds nothing neither reads nor writes its cells
        unsigned cw[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) cw[i] = 0u;
        const bool wide = cells_wide<CH>(nin, p0);
        unsigned short* cell0 = (FIRST && LAST) ? nullptr : cells + (int64_t)H * p0;
        if (!FIRST) cells_load<CH>(cell0, nin, wide, cw);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned add[H];
            const unsigned own = FIRST ? ((mr >> (8 * j)) & 1u) * kDenoiseW : 0u;
#pragma unroll
            for (int c = 0; c < CH; ++c) add[c] = own * byte_of(rw, CH * j + c) + wgt[j] * kk[j][c];
            add[CH] = own + wgt[j];
#pragma unroll
            for (int h = 0; h < H; ++h) cw[(H * j + h) >> 1] += add[h] << (16 * ((H * j + h) & 1));  // no halfword overflows: n <= 240, sums <= 61 200
        }
        if (!LAST) {
            cells_store<CH>(cell0, nin, wide, cw);
        } else {
            unsigned ow[CH], mw = 0u, nw = 0u;
#pragma unroll
            for (int d = 0; d < CH; ++d) ow[d] = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned n = half_of(cw, H * j + CH);
                const unsigned ok = n > 0u ? 1u : 0u, den = ok ? 2u * n : 1u;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const unsigned val = ok ? (2u * half_of(cw, H * j + c) + n) / den : 0u;  // round half up; <= 255
                    ow[(CH * j + c) >> 2] |= val << (8 * ((CH * j + c) & 3));
                }
                mw |= ok << (8 * j);
                nw |= (n & 0xffu) << (8 * j);
                if (j < nin) {
                    n3[0] += 1u - ok;
                    n3[1] += n == kDenoiseW ? 1u : 0u;
                    n3[2] += n > kDenoiseW ? 1u : 0u;
                }
            }
            unsigned char* const planes[2] = {mask_out, weight};
            const unsigned words[2] = {mw, nw};
            store_group<CH>(out, ow, planes, words, p0, nin);
        }
    }
    if constexpr (LAST) block_counts_add<3>(n3, counts);
}

}  // namespace

}  // namespace rsdsfm
