// deblur_sharpness_body.hpp -- the body of the sharpness transfer's sharpness kernels, included INSIDE the braces of deblur_sharpness_kernel<CH>
// (deblur_kernels.hip) and of deblur_band_sharpness_kernel<CH> (deblur_bands_kernels.hip); no include guard, no namespace.  A text and not a
// __forceinline__ function: as a function the compiler orders the instructions of deblur_sharpness_kernel differently from the kernel that carried
// this code itself (profiles/deblur_bands_isa.txt), and that kernel is to stay what it was.  Names it takes from the kernel: CH; ref, rmask, layer,
// lmask, rows, cols, sums, min_overlap, gain_mode; T, the record that gets [pairs, A_R, A_L] of the workgroup's tile.  Every pair goes to the
// record of its left or upper pixel's tile.  Described in deblur_kernels.hip's header.
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
