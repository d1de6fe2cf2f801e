// plate_medoid_kernels.hip -- the clean plate's colour-consistent estimator on MI355X (gfx950, wave64): include/rsdsfm_plate_medoid.h, defined by
// tests/plate_medoid_spec_numpy.py and reproduced bit for bit.  Where the median (plate_kernels.hip) selects every channel on its own, this one
// selects a whole candidate: the L1 medoid.  Integer arithmetic only; every value goes to memory through ordinary stores and atomicAdd.
//   plate_medoid_kernel<3, NL, FLAG>  on the 16 x 64 tile of image_tile_device.hpp, the median's PlateArgs, instance sizes (kPlateSizes = 0, 2, 4,
//                               7, 14), loads, gains and flag stage (plate_device.hpp): only the selection differs.  BGR only: with one channel
//                               the medoid IS the lower median, and the launcher runs plate_median_kernel.
//                               Selection, per pixel: the NL + 1 candidates as packed dwords b | g << 8 | r << 16 (the layers' bytes under
//                                 their gains), a candidate that is not there 0, and a validity bitmask.  Every ordered pair (i, j), i != j, is
//                                 one v_sad_u8 with the cost as its accumulator: cost_i += |b_i - b_j| + |g_i - g_j| + |r_i - r_j|, N (N - 1)
//                                 of them.  A candidate that is not there took part as 0 and gave every cost_i the sum b_i + g_i + r_i, one
//                                 more v_sad_u8 against 0; N - n of them are taken off again: what remains is the sum over the pairs of VALID
//                                 candidates, exactly.  Then cost-then-colour: the smallest cost among the valid (the others 0xFFFFFFFF), and
//                                 the smallest packed colour among the candidates of that cost -- the order of the key (cost << 24) | colour.
//                                 Fully unrolled, every index a compile-time constant: the arrays live in registers, there is no scratch
//                                 (tests/test_no_scratch_in_plate_medoid.py).
//                               FLAG: e = |R - P| summed over the channels is one v_sad_u8 of the two packed pixels.  A halo thread forms its own
//                                 medoid with the same routine from bytes it loads itself, never outside the frame.
//                               Every byte of the outputs given is written, no preset.  The bytes moved are the median's.
#include "plate_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace {

static_assert(kPlateSizes[kPlateNumSizes - 1] == kPlateLayersMax, "the largest instance holds every call");

constexpr unsigned kNoCost = 0xFFFFFFFFu;  // a candidate that is not there: above every cost (at most 14 * 765) and every packed colour (24 bits)

// sum over the four bytes of |a - b|, + acc: one v_sad_u8
__device__ __forceinline__ unsigned sad4(unsigned a, unsigned b, unsigned acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }

// pixel j's three bytes of a thread's three image dwords, as b | g << 8 | r << 16
__device__ __forceinline__ unsigned pixel_of(const unsigned* w, int j) {
    return j == 0 ? w[0] & 0xffffffu : j == 1 ? (w[0] >> 24) | ((w[1] & 0xffffu) << 8) : j == 2 ? (w[1] >> 16) | ((w[2] & 0xffu) << 16) : w[2] >> 8;
}

// a packed pixel under a layer's three gains
__device__ __forceinline__ unsigned gained3(const unsigned* G, unsigned px) {
    return gained(G[0], px & 0xffu) | (gained(G[1], (px >> 8) & 0xffu) << 8) | (gained(G[2], px >> 16) << 16);
}

// the packed colour of the L1 medoid of the candidates c[i] with bit i of `valid` set (c[i] == 0 where it is not; the top byte of every c[i] is
// 0): the smallest (cost, colour).  0 where valid == 0
template <int N>
__device__ __forceinline__ unsigned medoid_of(const unsigned (&c)[N], unsigned valid) {
    const unsigned absent = (unsigned)N - (unsigned)__popc(valid);
    unsigned cost[N];
#pragma unroll
    for (int i = 0; i < N; ++i) cost[i] = 0u;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = i + 1; j < N; ++j) {
            cost[i] = sad4(c[i], c[j], cost[i]);
            cost[j] = sad4(c[j], c[i], cost[j]);
        }
    unsigned best = kNoCost;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        cost[i] = ((valid >> i) & 1u) ? cost[i] - absent * sad4(c[i], 0u, 0u) : kNoCost;  // the absent candidates' share: each was a 0
        best = cost[i] < best ? cost[i] : best;
    }
    unsigned colour = kNoCost;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const unsigned k = cost[i] == best ? c[i] : kNoCost;
        colour = k < colour ? k : colour;
    }
    return valid ? colour : 0u;
}

template <int NL, bool FLAG>
__device__ __forceinline__ void plate_medoid_body(const PlateArgs& a) {
    constexpr int CH = 3, N = NL + 1;  // candidates
    __shared__ __attribute__((aligned(16))) unsigned s_tile[FLAG ? kTileLdsWords : 2];
    __shared__ unsigned s_gain[NL * CH + 1];
    const int rows = a.rows, cols = a.cols, nl = a.nlayers;
    const TileThread t = tile_thread(rows, cols);
    const int tid = t.tid, nin = t.nin;

    PlateLoads<CH, NL> l;
    plate_load<CH, NL>(a, t, l);
    plate_gains<CH, NL>(a, tid, s_gain);
    const unsigned mr = l.mr, nw = l.nw;

    // the medoids of the thread's own four pixels
    unsigned px[4] = {0u, 0u, 0u, 0u};
    if (nw) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned c[N], valid = (mr >> (8 * j)) & 1u;
            c[0] = valid ? pixel_of(l.rw, j) : 0u;
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const unsigned on = (l.ml[i] >> (8 * j)) & 1u;
                const unsigned G[CH] = {s_gain[i * CH], s_gain[i * CH + 1], s_gain[i * CH + 2]};
                c[1 + i] = on ? gained3(G, pixel_of(l.lw[i], j)) : 0u;
                valid |= on << (1 + i);
            }
            px[j] = medoid_of<N>(c, valid);
        }
    }
    const unsigned ow[CH] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
    const unsigned mw = bytes_set(nw);

    unsigned fw = 0u, n4[4] = {0u, 0u, 0u, 0u};  // the flags, a byte per pixel; [unset, static, moving, undecided], at most 4 per thread
    if constexpr (FLAG) {
        // stage 1: the packed (v, e) of the thread's own four pixels
        unsigned* row = tile_own(s_tile, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool v = ((mr >> (8 * j)) & 1u) && ((nw >> (8 * j)) & 0xffu) >= a.min_votes;
            row[j] = v ? (0x10000u | sad4(pixel_of(l.rw, j), px[j], 0u)) : 0u;
        }
        // the halo: one pixel per thread, its own medoid
        if (tid < kTileHalo) {
            const TileHalo h = tile_halo(t);
            unsigned ent = 0u;
            if (h.hy >= 0 && h.hy < rows && h.hx >= 0 && h.hx < cols) {
                const int64_t p = (int64_t)h.hy * cols + h.hx;
                if (a.rmask[p] != 0) {
                    unsigned valid = 1u, n = 1u;  // bit 1 + i: layer i saw the pixel
#pragma unroll
                    for (int i = 0; i < NL; ++i)
                        if (i < nl && a.lmask[i][p] != 0) {
                            valid |= 1u << (1 + i);
                            ++n;
                        }
                    if (n >= a.min_votes) {
                        unsigned c[N];
                        c[0] = (unsigned)a.ref[CH * p] | ((unsigned)a.ref[CH * p + 1] << 8) | ((unsigned)a.ref[CH * p + 2] << 16);
#pragma unroll
                        for (int i = 0; i < NL; ++i) {
                            c[1 + i] = 0u;
                            if ((valid >> (1 + i)) & 1u) {
                                const unsigned char* q = a.layer[i] + CH * p;
                                c[1 + i] = gained(s_gain[i * CH], q[0]) | (gained(s_gain[i * CH + 1], q[1]) << 8) | (gained(s_gain[i * CH + 2], q[2]) << 16);
                            }
                        }
                        ent = 0x10000u | sad4(c[0], medoid_of<N>(c, valid), 0u);
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
    store_group<CH>(a.out, ow, planes, words, t.p0, nin);

    if constexpr (FLAG) block_counts_add<4>(n4, a.counts);
}

}  // namespace

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  out, mask_out and votes (may be NULL) are written whole; FLAG: moving (may be NULL) is
// written whole and counts[0 .. 3] (may be NULL) += [unset, static, moving, undecided].  CH is 3: there are no gray instances
template <int CH, int NL, bool FLAG>
__global__ __launch_bounds__(kBP) void plate_medoid_kernel(const PlateArgs a) {
    static_assert(CH == 3, "with one channel the medoid is the lower median: plate_median_kernel");
    plate_medoid_body<NL, FLAG>(a);
}

// ---------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------
int plate_medoid_launch(Ctx* c, const PlateArgs& args, int channels) {
    if (channels == 1) return plate_median_launch(c, args, channels);  // the same bytes (tests/plate_medoid_spec_numpy.py, consequence (a))
    if (args.counts) RSDSFM_HIP_CHECK(c, hipMemsetAsync(args.counts, 0, 4 * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const PlateArgs);
    static const Kernel kernels[kPlateNumSizes][2] = {{plate_medoid_kernel<3, 0, false>, plate_medoid_kernel<3, 0, true>},
                                                      {plate_medoid_kernel<3, 2, false>, plate_medoid_kernel<3, 2, true>},
                                                      {plate_medoid_kernel<3, 4, false>, plate_medoid_kernel<3, 4, true>},
                                                      {plate_medoid_kernel<3, 7, false>, plate_medoid_kernel<3, 7, true>},
                                                      {plate_medoid_kernel<3, 14, false>, plate_medoid_kernel<3, 14, true>}};
    static_assert(kPlateSizes[0] == 0 && kPlateSizes[1] == 2 && kPlateSizes[2] == 4 && kPlateSizes[3] == 7 && kPlateSizes[4] == 14, "the table above");
    int size = 0;
    while (kPlateSizes[size] < args.nlayers) ++size;  // nlayers <= 14: checked by the caller
    const bool flag = args.moving != nullptr || args.counts != nullptr;
    hipLaunchKernelGGL(kernels[size][flag], tile_grid(args.rows, args.cols), dim3(kBP), 0, c->stream, args);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
