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
#include <algorithm>

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

template <int CH, bool FIRST, bool LAST>
__device__ __forceinline__ void deblur_accumulate_body(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                       const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                       const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode, unsigned strength,
                                                       const unsigned long long* __restrict__ sharp, int margin, long long min_pairs, int gate_mode,
                                                       unsigned short* __restrict__ cells, unsigned char* __restrict__ out, unsigned char* __restrict__ mask_out,
                                                       unsigned char* __restrict__ weight, unsigned long long* __restrict__ counts) {
    constexpr int H = CH + 1;     // halfwords per cell
    constexpr int NW = 4 * H / 2; // dwords of a thread's four cells: 8 (BGR) or 4 (gray)
    __shared__ __attribute__((aligned(16))) unsigned s_tile[kTileLdsWords];
    __shared__ unsigned s_gain[CH + 1];  // the gains, then tau
    const TileThread t = tile_thread(rows, cols);
    unsigned tau = 0u;
    if (layer != nullptr) {  // (uniform)
        if (t.tid < CH) s_gain[t.tid] = sums ? seam_gain(sums, CH, t.tid, min_overlap, gain_mode) : kGainOne;
        if (t.tid == CH) s_gain[CH] = deblur_tau_of(sharp, margin, min_pairs);
        __syncthreads();
        tau = s_gain[CH];
        if (!FIRST && !LAST && tau == 0u) return;  // (uniform) a layer that is no sharper adds nothing: no image byte is read
    }
    const bool has_layer = tau != 0u;  // (uniform)
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

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  T[0 .. 2] += [pairs, A_R, A_L] of the workgroup's tile (T zeroed by the caller)
template <int CH>
__global__ __launch_bounds__(kBP) void deblur_sharpness_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                              const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                              const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode,
                                                              unsigned long long* __restrict__ T) {
    __shared__ __attribute__((aligned(16))) unsigned s_tile[kTileLdsWords];
    __shared__ unsigned s_gain[CH];
    const TileThread t = tile_thread(rows, cols);
    const int nin = t.nin;
    const int64_t p0 = t.p0, npix = (int64_t)rows * cols;
    unsigned v = 0u;
    if (nin) {  // the mask dwords first
        unsigned w1[1];
        load_bytes<1>(rmask, p0, npix, w1);
        const unsigned mr = bytes_set(w1[0]) & first_ones(nin);
        if (mr) {
            load_bytes<1>(lmask, p0, npix, w1);
            v = bytes_set(w1[0]) & mr;
        }
    }
    if (t.tid < CH) s_gain[t.tid] = sums ? seam_gain(sums, CH, t.tid, min_overlap, gain_mode) : kGainOne;
    __syncthreads();
    unsigned G[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) G[c] = s_gain[c];
    unsigned ent[4] = {0u, 0u, 0u, 0u};
    if (v) {  // image bytes only where a pixel has both masks
        unsigned rw[CH], lw[CH];
        load_bytes<CH>(ref, (int64_t)CH * p0, (int64_t)CH * npix, rw);
        load_bytes<CH>(layer, (int64_t)CH * p0, (int64_t)CH * npix, lw);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned yr = 0u, yl = 0u;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                yr += byte_of(rw, CH * j + c);
                yl += gained(G[c], byte_of(lw, CH * j + c));
            }
            ent[j] = ((v >> (8 * j)) & 1u) ? (kSharpV | (yr << 10) | yl) : 0u;
        }
    }
    unsigned* row = tile_own(s_tile, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) row[j] = ent[j];
    if (t.tid < kTileHalo) {
        const TileHalo h = tile_halo(t);
        // only the column to the right and the row below are read
        const bool below = h.ly == kTileRows + 1 && h.lx >= 1 && h.lx <= kTileCols, right = h.lx == kTileCols + 1 && h.ly >= 1 && h.ly <= kTileRows;
        if (below || right) {
            unsigned e = 0u;
            if (h.hy < rows && h.hx < cols) {  // both are >= 0 here
                const int64_t p = (int64_t)h.hy * cols + h.hx;
                if (rmask[p] != 0 && lmask[p] != 0) {
                    unsigned yr = 0u, yl = 0u;
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        yr += ref[CH * p + c];
                        yl += gained(G[c], layer[CH * p + c]);
                    }
                    e = kSharpV | (yr << 10) | yl;
                }
            }
            s_tile[h.ly * kTileLdsStride + h.lx] = e;
        }
    }
    __syncthreads();
    unsigned n3[3] = {0u, 0u, 0u};  // [pairs, A_R, A_L] of the thread's four pixels
    if (v) {
        // 8-byte reads as tile_sum3x3's: the row below as [4 g .. 4 g + 5] (its first and last dword are not used), the right neighbour in [4 g + 4, 4 g + 5]
        const Lds8* lo = static_cast<const Lds8*>(__builtin_assume_aligned(s_tile + (t.ty + 2) * kTileLdsStride + 4 * t.g, 8));
        const Lds8* own = static_cast<const Lds8*>(__builtin_assume_aligned(s_tile + (t.ty + 1) * kTileLdsStride + 4 * t.g + 4, 8));
        const Lds8 b0 = lo[0], b1 = lo[1], b2 = lo[2];
        const unsigned right = own[0][1];
        const unsigned down[4] = {b0[1], b1[0], b1[1], b2[0]};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ent[j]) {
                sharp_pair(ent[j], j < 3 ? ent[(j + 1) & 3] : right, n3);
                sharp_pair(ent[j], down[j], n3);
            }
    }
    // a workgroup's largest sum: 2 pairs x 1024 pixels x 765^2 = 1 198 540 800 < 2^32, so the 32-bit sums of block_counts_add are exact
    block_counts_add<3>(n3, T);
}

template <int CH, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBP) void deblur_accumulate_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                               const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                               const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode, unsigned strength,
                                                               const unsigned long long* __restrict__ sharp, int margin, long long min_pairs, int gate_mode,
                                                               unsigned short* __restrict__ cells, unsigned char* __restrict__ out,
                                                               unsigned char* __restrict__ mask_out, unsigned char* __restrict__ weight,
                                                               unsigned long long* __restrict__ counts) {
    deblur_accumulate_body<CH, FIRST, LAST>(ref, rmask, layer, lmask, rows, cols, sums, min_overlap, gain_mode, strength, sharp, margin, min_pairs, gate_mode, cells, out,
                                            mask_out, weight, counts);
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
