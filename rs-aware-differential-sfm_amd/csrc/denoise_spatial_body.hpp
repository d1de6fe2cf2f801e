// denoise_spatial_body.hpp -- the body of the spatial top-up's kernels, included INSIDE the braces of denoise_spatial_kernel<CH, S>
// (denoise_spatial_kernels.hip), of denoise_spatial_auto_kernel<CH, S> (noise_kernels.hip) and of denoise_spatial_curve_kernel<CH, S>
// (noise_curve_kernels.hip); no include guard, no namespace.  A text and not a __forceinline__ function, as deblur_sharpness_body.hpp is and for
// its reason: as a function the compiler orders the instructions of denoise_spatial_kernel differently from the kernel that carried this code
// itself, and that kernel is to stay what it was.  Names it takes from the kernel: CH, S; image, mask, weight, rows, cols, target, out, support,
// counts, and the divisor's strength through two macros, which this text undefines at its end:
//   RSDSFM_SPATIAL_HN_SETUP   statements behind the fill of the tile (pk[0 .. 3], the thread's packed centre pixels, are in scope) that declare hn
//   RSDSFM_SPATIAL_HN(j)      the strength of the thread's pixel j, times CH
// (the launch's one strength: `const unsigned hn = strength * (unsigned)CH;` and `hn`; a strength per pixel: hn[4] and `hn[j]`).  out and support
// (may be NULL) are written whole; counts[0 .. 2] (may be NULL) += [unset, kept, smoothed].  weight == NULL: n = 16 where the mask is set.
// Described in denoise_spatial_kernels.hip's header; SpatialLds, kSetBit and pair_entry are denoise_spatial_device.hpp's.
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
        RSDSFM_SPATIAL_HN_SETUP
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
                            const unsigned qd = (kDenoiseW * (s & 0xffffu)) / (RSDSFM_SPATIAL_HN(j) * (s >> 16));
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
#undef RSDSFM_SPATIAL_HN_SETUP
#undef RSDSFM_SPATIAL_HN
