// noise_temporal_kernels.hip -- the temporal noise curve on MI355X (gfx950, wave64): include/rsdsfm_noise_temporal.h, defined by
// tests/noise_temporal_spec_numpy.py and reproduced bit for bit.  Integer arithmetic only; every value goes to memory through ordinary stores
// and atomicAdd.
//   noise_pair_hist_kernel<CH>   the toolkit's 16 x 64 tile (image_tile_device.hpp), 256 threads of 4 pixels.
//                                Stage 1 is the denoise accumulate's: the reference's and the layer's mask dwords first, image bytes only where
//                                v is set, one packed dword per pixel, e | v << 16 | clipped << 24, into the tile's 18 x 66 dwords of LDS with
//                                the halo of 1 formed by threads 0 .. 163.  Over nine pixels the fields cannot carry: e <= 6885 < 2^16, the
//                                counts <= 9.
//                                Stage 2 is tile_sum3x3 on that plane: D, C and X of the thread's four pixels from one 3 x 6 window.
//                                Stage 3 is the noise curve's histogram: ONE LDS array of 8 x 1024 uint32 (32 KB beside the plane's 4 752 B, so
//                                LDS admits four workgroups per CU), an LDS atomic per sample at band << 10 | bin, then one global 32-bit
//                                atomicAdd per non-zero bin and workgroup, every thread reading its 32 words.
//                                A workgroup whose tile holds no v pixel has no sample (a sample's window is full, so the pixel itself is set):
//                                it leaves behind the first barrier, which carries the vote, and neither zeroes nor flushes the table.
//                                The divisions by 256 N are by the compile-time constants 2304 and 6912.
// The resolve is noise_curve_kernels.hip's noise_curve_resolve_kernel, launched here through its declaration in noise_temporal.hpp.
#include "image_tile_device.hpp"
#include "noise_temporal.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace {

static_assert(kNoiseBins == 1024 && kCurveHistWords % kBP == 0, "a key is band << 10 | bin; a thread of the workgroup owns kCurveHistWords / kBP words");

// 1 in every byte of w that is 0 or 255
__device__ __forceinline__ unsigned pair_bytes_clipped(unsigned w) { return bytes_zero(w) | bytes_zero(~w); }

// x / 3 for x <= 766 as a multiply-shift (tests/test_noise_curve_cpu.py proves it exact)
__device__ __forceinline__ unsigned pair_third(unsigned x) { return (x * 21846u) >> 16; }

// 1 when any of pixel j's CH bytes in the packed flags (one flag byte per image byte) is set
template <int CH>
__device__ __forceinline__ unsigned pixel_any(const unsigned* flags, int j) {
    unsigned a = 0u;
#pragma unroll
    for (int c = 0; c < CH; ++c) a |= byte_of(flags, CH * j + c);
    return a & 1u;
}

}  // namespace

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  hist (8 x 1024 words, zeroed by the caller's first step) += the workgroup's histogram
template <int CH>
__global__ __launch_bounds__(kBP) void noise_pair_hist_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                             const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                             const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode,
                                                             unsigned* __restrict__ hist) {
    constexpr unsigned N = 9u * (unsigned)CH;
    __shared__ __attribute__((aligned(16))) unsigned s_tile[kTileLdsWords];
    __shared__ unsigned s_hist[kCurveHistWords];
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
    if (!__syncthreads_or(v != 0u)) return;  // (uniform) no v pixel in the tile: no sample, the table neither zeroed nor flushed

#pragma unroll
    for (int k = 0; k < kCurveHistWords / kBP; ++k) s_hist[t.tid + k * kBP] = 0u;
    unsigned G[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) G[c] = s_gain[c];

    // stage 1: the thread's own four pixels
    unsigned rw[CH], ent[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < CH; ++d) rw[d] = 0u;
    if (v) {  // image bytes under an empty mask are not read
        unsigned lw[CH], clip[CH];
        load_bytes<CH>(ref, (int64_t)CH * p0, (int64_t)CH * npix, rw);
        load_bytes<CH>(layer, (int64_t)CH * p0, (int64_t)CH * npix, lw);
#pragma unroll
        for (int d = 0; d < CH; ++d) clip[d] = pair_bytes_clipped(rw[d]) | pair_bytes_clipped(lw[d]);  // of the layer BEFORE the gain
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned e = 0u;
#pragma unroll
            for (int c = 0; c < CH; ++c) e += absdiff(byte_of(rw, CH * j + c), gained(G[c], byte_of(lw, CH * j + c)));
            ent[j] = ((v >> (8 * j)) & 1u) ? (e | 0x10000u | (pixel_any<CH>(clip, j) << 24)) : 0u;
        }
    }
    unsigned* own = tile_own(s_tile, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) own[j] = ent[j];
    if (t.tid < kTileHalo) {
        const TileHalo h = tile_halo(t);
        unsigned e = 0u;
        if (h.hy >= 0 && h.hy < rows && h.hx >= 0 && h.hx < cols) {
            const int64_t p = (int64_t)h.hy * cols + h.hx;
            if (rmask[p] != 0 && lmask[p] != 0) {
                e = 0x10000u;
                unsigned cl = 0u;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const unsigned r = ref[CH * p + c], l = layer[CH * p + c];
                    e += absdiff(r, gained(G[c], l));
                    cl |= (r == 0u || r == 255u || l == 0u || l == 255u) ? 1u : 0u;
                }
                e |= cl << 24;
            }
        }
        s_tile[h.ly * kTileLdsStride + h.lx] = e;
    }
    __syncthreads();

    // stage 2: the 3 x 3 sums of the packed dwords; stage 3: a sample's key into the workgroup's table
    if (v) {
        unsigned col[6];
        tile_sum3x3(s_tile, t.ty, t.g, col);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned s = col[j] + col[j + 1] + col[j + 2];
            const unsigned D = s & 0xffffu, C = (s >> 16) & 0xffu, X = s >> 24;
            if (C == 9u && X == 0u) {  // a full window: the pixel itself is set and inside the frame
                unsigned lvl = byte_of(rw, CH * j);
                if constexpr (CH == 3) lvl = pair_third(lvl + byte_of(rw, CH * j + 1) + byte_of(rw, CH * j + 2) + 1u);
                const unsigned bin = (kPairBinNum * D + 128u * N) / (256u * N);  // <= 914
                atomicAdd(&s_hist[((lvl >> 5) << 10) | bin], 1u);
            }
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kCurveHistWords / kBP; ++k) {
        const unsigned n = s_hist[t.tid + k * kBP];
        if (n) atomicAdd(hist + t.tid + k * kBP, n);
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int noise_pair_hist_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels, int rows,
                           int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, bool first, unsigned* d_hist) {
    if (first) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_hist, 0, kCurveHistWords * sizeof(unsigned), c->stream));
    if (channels == 3)
        hipLaunchKernelGGL(noise_pair_hist_kernel<3>, tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_ref, d_rmask, d_layer, d_lmask, rows, cols, d_sums,
                           (long long)min_overlap, gain_mode, d_hist);
    else
        hipLaunchKernelGGL(noise_pair_hist_kernel<1>, tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_ref, d_rmask, d_layer, d_lmask, rows, cols, d_sums,
                           (long long)min_overlap, gain_mode, d_hist);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int noise_curve_resolve_launch(Ctx* c, const unsigned* d_hist, int quantile, unsigned long long* d_curve) {
    hipLaunchKernelGGL(noise_curve_resolve_kernel, dim3(kCurveRows), dim3(kBP), 0, c->stream, d_hist, (unsigned)quantile, d_curve);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
