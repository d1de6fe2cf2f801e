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
#include "image_tile_device.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace {

template <int CH, bool FIRST, bool LAST>
__device__ __forceinline__ void denoise_accumulate_body(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                        const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                        const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode, unsigned strength,
                                                        unsigned short* __restrict__ cells, unsigned char* __restrict__ out, unsigned char* __restrict__ mask_out,
                                                        unsigned char* __restrict__ weight, unsigned long long* __restrict__ counts) {
    constexpr int H = CH + 1;     // halfwords per cell
    constexpr int NW = 4 * H / 2; // dwords of a thread's four cells: 8 (BGR) or 4 (gray)
    __shared__ __attribute__((aligned(16))) unsigned s_tile[kTileLdsWords];
    __shared__ unsigned s_gain[CH];
    const bool has_layer = layer != nullptr;  // (uniform)
    const TileThread t = tile_thread(rows, cols);
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
        if (t.tid < CH) s_gain[t.tid] = sums ? seam_gain(sums, CH, t.tid, min_overlap, gain_mode) : kGainOne;
        __syncthreads();
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
                unsigned e = 0u;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    kk[j][c] = gained(G[c], byte_of(lw, CH * j + c));
                    e += absdiff(byte_of(rw, CH * j + c), kk[j][c]);
                }
                ent[j] = ((v >> (8 * j)) & 1u) ? (0x10000u | e) : 0u;
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
                    e = 0x10000u;
#pragma unroll
                    for (int c = 0; c < CH; ++c) e += absdiff(ref[CH * p + c], gained(G[c], layer[CH * p + c]));
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
                const unsigned D = s & 0xffffu, cnt = s >> 16;
                if ((v >> (8 * j)) & 1u) {  // the pixel itself counts: cnt >= 1
                    const unsigned qd = (kDenoiseW * D) / (strength * (unsigned)CH * cnt);
                    wgt[j] = kDenoiseW - (qd > kDenoiseW ? kDenoiseW : qd);
                }
            }
        }
    }

    unsigned n3[3] = {0u, 0u, 0u};  // [unset, own only, averaged]; at most 4 per thread
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
