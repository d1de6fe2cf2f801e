// plate_device.hpp -- what the clean plate's two estimators share on the device (plate_kernels.hip: the per-channel median; plate_medoid_kernels.hip:
// the L1 medoid): the loads, the gains and the flag stage are the same code, only the selection between them differs.  Every function is
// __device__ __forceinline__ on the 16 x 64 tile of image_tile_device.hpp, so a kernel built from these blocks is the code it was when it
// carried its own copy.
#pragma once

#include "image_tile_device.hpp"
#include "plate.hpp"
#include "rectify_dense_device.hpp"

namespace rsdsfm {

// a thread's four pixels as they come from memory: the mask bytes as 1 / 0 per pixel (mr the reference's, ml[j] layer j's), the votes nw (a
// byte per pixel: at most 15, no carry) and the image dwords (rw, lw[j]; 0 where nothing was read).  ml[NL] and lw[NL] are never used: no array
// of length 0
template <int CH, int NL>
struct PlateLoads {
    unsigned mr, nw, ml[NL + 1], rw[CH], lw[NL + 1][CH];
};

// the NL + 1 mask dwords first, then an image's CH dwords only where one of its four mask bytes is set: image bytes under an empty mask are not read
template <int CH, int NL>
__device__ __forceinline__ void plate_load(const PlateArgs& a, const TileThread& t, PlateLoads<CH, NL>& l) {
    const int nl = a.nlayers;
    const int64_t p0 = t.p0, npix = (int64_t)a.rows * a.cols;
    const unsigned inside = first_ones(t.nin);
    l.mr = 0u;
#pragma unroll
    for (int j = 0; j < NL; ++j) l.ml[j] = 0u;
    if (t.nin) {
        unsigned w1[1];
        load_bytes<1>(a.rmask, p0, npix, w1);
        l.mr = bytes_set(w1[0]) & inside;
#pragma unroll
        for (int j = 0; j < NL; ++j)
            if (j < nl) {
                load_bytes<1>(a.lmask[j], p0, npix, w1);
                l.ml[j] = bytes_set(w1[0]) & inside;
            }
    }
    l.nw = l.mr;
#pragma unroll
    for (int j = 0; j < NL; ++j) l.nw += l.ml[j];
#pragma unroll
    for (int d = 0; d < CH; ++d) l.rw[d] = 0u;
    if (l.mr) load_bytes<CH>(a.ref, (int64_t)CH * p0, (int64_t)CH * npix, l.rw);
#pragma unroll
    for (int j = 0; j < NL; ++j) {
#pragma unroll
        for (int d = 0; d < CH; ++d) l.lw[j][d] = 0u;
        if (l.ml[j]) load_bytes<CH>(a.layer[j], (int64_t)CH * p0, (int64_t)CH * npix, l.lw[j]);
    }
}

// threads 0 .. NL CH - 1 compute seam_gain(record j, channel c) into s_gain[j CH + c], one barrier; nothing at NL == 0.  No host wait behind
// the sums kernels.  Every thread of the workgroup calls it
template <int CH, int NL>
__device__ __forceinline__ void plate_gains(const PlateArgs& a, int tid, unsigned* s_gain) {
    if constexpr (NL > 0) {
        if (tid < NL * CH) {
            const int j = tid / CH, c = tid % CH;
            s_gain[tid] = (a.sums && j < a.nlayers) ? seam_gain(a.sums + 8 * j, CH, c, a.min_overlap, a.gain_mode) : kGainOne;
        }
        __syncthreads();
    }
}

// the flag's second stage, behind the barrier that follows the packed (v << 16) | e of the tile and its halo in s_tile: the 3 x 3 sums, the
// flags of the thread's four pixels (fw, a byte per pixel) and what they add to [unset, static, moving, undecided] (n4, at most 4 per thread)
template <int CH>
__device__ __forceinline__ void plate_flags(const unsigned* s_tile, const TileThread& t, unsigned mr, unsigned threshold, unsigned& fw, unsigned (&n4)[4]) {
    if (mr) {
        unsigned col[6];
        tile_sum3x3(s_tile, t.ty, t.g, col);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned s = col[j] + col[j + 1] + col[j + 2];
            const unsigned D = s & 0xffffu, cnt = s >> 16;
            const unsigned f = cnt == 0u ? 3u : D > threshold * (unsigned)CH * cnt ? 2u : 1u;  // at most 255 * 27: products of integers, no division
            fw |= (((mr >> (8 * j)) & 1u) ? f : 0u) << (8 * j);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < t.nin) {
            const unsigned f = (fw >> (8 * j)) & 0xffu;
            n4[0] += f == 0u ? 1u : 0u;
            n4[1] += f == 1u ? 1u : 0u;
            n4[2] += f == 2u ? 1u : 0u;
            n4[3] += f == 3u ? 1u : 0u;
        }
}

}  // namespace rsdsfm
