// denoise_accumulate_body.hpp -- the body of the temporal denoise's accumulate, included INSIDE the braces of denoise_accumulate_body
// (denoise_device.hpp: the function denoise_accumulate_kernel and denoise_accumulate_auto_kernel call, with the launch's one strength) and of
// denoise_accumulate_curve_kernel<CH, FIRST, LAST> (noise_curve_kernels.hip, with a strength per pixel); no include guard, no namespace.  A text,
// as denoise_spatial_body.hpp is and for its reason: every kernel gets the tokens it had when it carried this code itself, so each compiles to
// the instructions it had.  Names it takes from where it stands: CH, FIRST, LAST; ref, rmask, layer, lmask, rows, cols, sums, min_overlap,
// gain_mode, cells, out, mask_out, weight, counts, and the strength through two macros, which this text undefines at its end:
//   RSDSFM_ACCUMULATE_TABLE         statements in front of the gain barrier, reached only when there is a layer (nothing; or the table in LDS)
//   RSDSFM_ACCUMULATE_STRENGTH(j)   the strength of the thread's pixel j in stage 2's divisor, >= 1 (rw, the reference's packed bytes, is in scope)
// The stages, the bytes and the counters are described at the head of denoise_kernels.hip.
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
        RSDSFM_ACCUMULATE_TABLE  // without a layer no weight is formed: no table
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
                    const unsigned qd = (kDenoiseW * D) / (RSDSFM_ACCUMULATE_STRENGTH(j) * (unsigned)CH * cnt);
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
#undef RSDSFM_ACCUMULATE_TABLE
#undef RSDSFM_ACCUMULATE_STRENGTH
