// plate_kernels.hip -- the clean plate's median on MI355X (gfx950, wave64): include/rsdsfm_plate.h, defined by tests/plate_spec_numpy.py and
// reproduced bit for bit.  Integer arithmetic only; every value goes to memory through ordinary stores and atomicAdd.  The project's first image
// stage that is not a sum: of the accumulate kernels (denoise_kernels.hip) only the tile is borrowed.
//   plate_median_kernel<CH, NL, FLAG>  on the 16 x 64 tile of image_tile_device.hpp (the plane reads, the LDS layout and its bank argument, the
//                               output group and the counters are described there).  The loads, the gains and the flag's second stage are
//                               plate_device.hpp's, shared with the L1 medoid (plate_medoid_kernels.hip): only the selection is this file's.
//                               NL: the layer count the instance is compiled for, one of kPlateSizes = 0, 2, 4, 7, 14; a call
//                               with L layers runs the smallest NL >= L and tests j < L (uniform) before it touches layer j.  The reference, the
//                               layers and the records are pointers in the kernel argument (PlateArgs, 320 B): after unrolling every one is a
//                               scalar load at a constant offset, there is no pointer table in memory.
//                               Loads: the NL + 1 mask dwords first; an image's CH dwords only where one of its four mask bytes is set.
//                               Gains: threads 0 .. NL CH - 1 compute seam_gain(record j, channel c) into LDS, one barrier; no host wait behind
//                                 the sums kernels.
//                               Selection, per channel and PAIR of pixels (pixel 0 with 2, 1 with 3): the NL + 1 candidates as packed halfwords,
//                                 an unset candidate 0xFFFF, sorted by Batcher's odd-even merge network for NL + 1 elements (59 compare-exchanges
//                                 at 15, 19 at 8, 9 at 5, 3 at 3), fully unrolled, every index a compile-time constant -- the array lives in
//                                 registers, there is no scratch (tests/test_no_scratch_in_plate.py).  A compare-exchange is one v_pk_min_u16 and
//                                 one v_pk_max_u16 on both pixels at once; the comparators the median does not depend on are removed by the
//                                 compiler.  The element at (n - 1) >> 1 is taken per halfword by a chain of selects over indices
//                                 0 .. NL / 2, not by indexing.
//                               FLAG (a flag plane or the counters were passed): e = sum_c |R_c - P_c| where mR is set and n >= min_votes, the
//                                 packed dword (v << 16) | e to LDS.  A halo thread forms its own median byte by byte (channels 0 and 1 share
//                                 the packed network), never outside the frame.  D > threshold * CH * count of the 3 x 3 sums decides.  The
//                                 four counters [unset, static, moving, undecided].
//                               Not FLAG: no LDS tile, no halo, one barrier (the gains; none at NL == 0).
//                               Every byte of the outputs given is written, no preset.
//                               BGR, five sources: 5 (3 + 1) = 20 B read and 3 + 1 (+ 1 + 1) B written per pixel, plus the halo's 164 / 1024 of
//                                 the reads with FLAG.
#include <algorithm>

#include "plate_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace {

static_assert(kPlateSizes[kPlateNumSizes - 1] == kPlateLayersMax, "the largest instance holds every call");

constexpr unsigned kUnset = 0xFFFFu;  // a candidate that is not there: above every byte, so it sorts last

typedef unsigned short Half2 __attribute__((ext_vector_type(2)));  // two candidates of one compare-exchange

// Batcher's odd-even merge sort for N elements as a list of compare-exchanges (a[i] < b[i]), made at compile time
template <int N>
struct Network {
    int count = 0;
    int a[N * 5 + 1] = {}, b[N * 5 + 1] = {};  // 59 at N = 15
};

template <int N>
constexpr Network<N> make_network() {
    Network<N> net;
    for (int p = 1; p < N; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j <= N - 1 - k; j += 2 * k)
                for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        net.a[net.count] = i + j;
                        net.b[net.count] = i + j + k;
                        ++net.count;
                    }
    return net;
}

// both halfwords of a and b ordered: a the smaller, b the larger of each
__device__ __forceinline__ void compare_exchange(unsigned& a, unsigned& b) {
    const Half2 x = __builtin_bit_cast(Half2, a), y = __builtin_bit_cast(Half2, b);
    a = __builtin_bit_cast(unsigned, __builtin_elementwise_min(x, y));
    b = __builtin_bit_cast(unsigned, __builtin_elementwise_max(x, y));
}

template <int N, int I>
__device__ __forceinline__ void network_from(unsigned (&v)[N]) {
    constexpr Network<N> net = make_network<N>();
    if constexpr (I < net.count) {
        constexpr int ia = net.a[I], ib = net.b[I];
        compare_exchange(v[ia], v[ib]);
        network_from<N, I + 1>(v);
    }
}

// the packed lower medians of the N candidates of two pixels (low and high halfwords; an unset candidate is kUnset): the elements at med_lo and
// med_hi (each (n - 1) >> 1 <= (N - 1) / 2) of the ascending orders, as (low | high << 16)
template <int N>
__device__ __forceinline__ unsigned median2(unsigned (&v)[N], unsigned med_lo, unsigned med_hi) {
    network_from<N, 0>(v);
    unsigned lo = v[0] & 0xffffu, hi = v[0] >> 16;
#pragma unroll
    for (int i = 1; i <= (N - 1) / 2; ++i) {
        lo = med_lo == (unsigned)i ? (v[i] & 0xffffu) : lo;
        hi = med_hi == (unsigned)i ? (v[i] >> 16) : hi;
    }
    return lo | (hi << 16);
}

template <int CH, int NL, bool FLAG>
__device__ __forceinline__ void plate_median_body(const PlateArgs& a) {
    constexpr int N = NL + 1;  // candidates
    __shared__ __attribute__((aligned(16))) unsigned s_tile[FLAG ? kTileLdsWords : 2];
    __shared__ unsigned s_gain[NL * CH + 1];
    const int rows = a.rows, cols = a.cols, nl = a.nlayers;
    const TileThread t = tile_thread(rows, cols);
    const int tid = t.tid, nin = t.nin;
    const int64_t p0 = t.p0;

    // the mask dwords first, then the images whose mask has a byte set; the gains (plate_device.hpp)
    PlateLoads<CH, NL> l;
    plate_load<CH, NL>(a, t, l);
    plate_gains<CH, NL>(a, tid, s_gain);
    const unsigned mr = l.mr, nw = l.nw;
    const unsigned (&ml)[N] = l.ml, (&rw)[CH] = l.rw, (&lw)[N][CH] = l.lw;

    // the medians of the thread's own four pixels: per channel, pixels 0 and 2, then 1 and 3
    unsigned ow[CH], med[4];
#pragma unroll
    for (int d = 0; d < CH; ++d) ow[d] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned n = (nw >> (8 * j)) & 0xffu;
        med[j] = n ? (n - 1u) >> 1 : 0u;
    }
    if (nw) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            unsigned G[N];
#pragma unroll
            for (int j = 0; j < NL; ++j) G[j] = s_gain[j * CH + c];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                unsigned v[N];
                v[0] = (((mr >> (8 * h)) & 1u) ? byte_of(rw, CH * h + c) : kUnset) | ((((mr >> (8 * (h + 2))) & 1u) ? byte_of(rw, CH * (h + 2) + c) : kUnset) << 16);
#pragma unroll
                for (int j = 0; j < NL; ++j)
                    v[1 + j] = (((ml[j] >> (8 * h)) & 1u) ? gained(G[j], byte_of(lw[j], CH * h + c)) : kUnset) |
                               ((((ml[j] >> (8 * (h + 2))) & 1u) ? gained(G[j], byte_of(lw[j], CH * (h + 2) + c)) : kUnset) << 16);
                const unsigned m2 = median2<N>(v, med[h], med[h + 2]);
                const unsigned lo = ((nw >> (8 * h)) & 0xffu) ? (m2 & 0xffu) : 0u, hi = ((nw >> (8 * (h + 2))) & 0xffu) ? ((m2 >> 16) & 0xffu) : 0u;
                ow[(CH * h + c) >> 2] |= lo << (8 * ((CH * h + c) & 3));
                ow[(CH * (h + 2) + c) >> 2] |= hi << (8 * ((CH * (h + 2) + c) & 3));
            }
        }
    }
    const unsigned mw = bytes_set(nw);

    unsigned fw = 0u, n4[4] = {0u, 0u, 0u, 0u};  // the flags, a byte per pixel; [unset, static, moving, undecided], at most 4 per thread
    if constexpr (FLAG) {
        // stage 1: the packed (v, e) of the thread's own four pixels
        unsigned* row = tile_own(s_tile, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned e = 0u;
#pragma unroll
            for (int c = 0; c < CH; ++c) e += absdiff(byte_of(rw, CH * j + c), byte_of(ow, CH * j + c));
            const bool v = ((mr >> (8 * j)) & 1u) && ((nw >> (8 * j)) & 0xffu) >= a.min_votes;
            row[j] = v ? (0x10000u | e) : 0u;
        }
        // the halo: one pixel per thread, its own median
        if (tid < kTileHalo) {
            const TileHalo h = tile_halo(t);
            unsigned ent = 0u;
            if (h.hy >= 0 && h.hy < rows && h.hx >= 0 && h.hx < cols) {
                const int64_t p = (int64_t)h.hy * cols + h.hx;
                if (a.rmask[p] != 0) {
                    unsigned seen = 0u, n = 1u;  // bit j: layer j saw the pixel
#pragma unroll
                    for (int j = 0; j < NL; ++j)
                        if (j < nl && a.lmask[j][p] != 0) {
                            seen |= 1u << j;
                            ++n;
                        }
                    if (n >= a.min_votes) {
                        const unsigned mi = (n - 1u) >> 1;
                        unsigned R[CH], P[CH], k[N][CH];
#pragma unroll
                        for (int c = 0; c < CH; ++c) R[c] = a.ref[CH * p + c];
#pragma unroll
                        for (int j = 0; j < NL; ++j)
#pragma unroll
                            for (int c = 0; c < CH; ++c) k[j][c] = ((seen >> j) & 1u) ? gained(s_gain[j * CH + c], a.layer[j][CH * p + c]) : kUnset;
#pragma unroll
                        for (int c = 0; c < CH; c += 2) {  // channels c and c + 1 share the packed network
                            const bool two = c + 1 < CH;
                            unsigned v[N];
                            v[0] = R[c] | ((two ? R[c + 1 < CH ? c + 1 : c] : kUnset) << 16);
#pragma unroll
                            for (int j = 0; j < NL; ++j) v[1 + j] = k[j][c] | ((two ? k[j][c + 1 < CH ? c + 1 : c] : kUnset) << 16);
                            const unsigned m2 = median2<N>(v, mi, two ? mi : 0u);
                            P[c] = m2 & 0xffffu;
                            if (two) P[c + 1 < CH ? c + 1 : c] = m2 >> 16;
                        }
                        ent = 0x10000u;
#pragma unroll
                        for (int c = 0; c < CH; ++c) ent += absdiff(R[c], P[c]);
                    }
                }
            }
            s_tile[h.ly * kTileLdsStride + h.lx] = ent;
        }
        __syncthreads();
        // stage 2: the 3 x 3 sums of the packed dwords
        plate_flags<CH>(s_tile, t, mr, a.threshold, fw, n4);
    }

    unsigned char* const planes[3] = {a.mask_out, a.votes, FLAG ? a.moving : nullptr};
    const unsigned words[3] = {mw, nw, fw};
    store_group<CH>(a.out, ow, planes, words, p0, nin);

    if constexpr (FLAG) block_counts_add<4>(n4, a.counts);
}

}  // namespace

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  out, mask_out and votes (may be NULL) are written whole; FLAG: moving (may be NULL) is
// written whole and counts[0 .. 3] (may be NULL) += [unset, static, moving, undecided]
template <int CH, int NL, bool FLAG>
__global__ __launch_bounds__(kBP) void plate_median_kernel(const PlateArgs a) {
    plate_median_body<CH, NL, FLAG>(a);
}

// ---------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------
int plate_median_launch(Ctx* c, const PlateArgs& args, int channels) {
    if (args.counts) RSDSFM_HIP_CHECK(c, hipMemsetAsync(args.counts, 0, 4 * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const PlateArgs);
#define RSDSFM_PLATE_ROW(CH) \
    {{plate_median_kernel<CH, 0, false>, plate_median_kernel<CH, 0, true>}, {plate_median_kernel<CH, 2, false>, plate_median_kernel<CH, 2, true>}, \
     {plate_median_kernel<CH, 4, false>, plate_median_kernel<CH, 4, true>}, {plate_median_kernel<CH, 7, false>, plate_median_kernel<CH, 7, true>}, \
     {plate_median_kernel<CH, 14, false>, plate_median_kernel<CH, 14, true>}}
    static const Kernel kernels[2][kPlateNumSizes][2] = {RSDSFM_PLATE_ROW(1), RSDSFM_PLATE_ROW(3)};
#undef RSDSFM_PLATE_ROW
    static_assert(kPlateSizes[0] == 0 && kPlateSizes[1] == 2 && kPlateSizes[2] == 4 && kPlateSizes[3] == 7 && kPlateSizes[4] == 14, "the table above");
    int size = 0;
    while (kPlateSizes[size] < args.nlayers) ++size;  // nlayers <= 14: checked by the caller
    const bool flag = args.moving != nullptr || args.counts != nullptr;
    hipLaunchKernelGGL(kernels[channels == 3][size][flag], tile_grid(args.rows, args.cols), dim3(kBP), 0, c->stream, args);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
