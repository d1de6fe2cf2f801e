// noise_curve_kernels.hip -- the noise curve on MI355X (gfx950, wave64): include/rsdsfm_noise_curve.h, defined by tests/noise_curve_spec_numpy.py
// and reproduced bit for bit.  Integer arithmetic only; every value goes to memory through ordinary stores and atomicAdd.
//   noise_curve_hist_kernel<CH>   noise_hist_kernel's tile, fill, window and separable K (noise_kernels.hip), unchanged, with the vertical and
//                                 horizontal [1, 1, 1] sums per channel beside the [1, -2, 1] ones, from the same window registers: S, the sum
//                                 of the sample's nine bytes, L = (S + 4) / 9 as a multiply-shift (exact for every S <= 2295;
//                                 tests/test_noise_curve_cpu.py) and the band L >> 5.
//                                 Histogram: ONE LDS array of 8 x 1024 uint32 (32 KB static beside the plane's 4 752 B: 37 520 B, so LDS admits
//                                 four workgroups per CU); a sample's key is band << 10 | bin.  The register combine of equal keys stays: a
//                                 flat frame is still one LDS atomic per thread.
//                                 Flush: one global 32-bit atomicAdd per non-zero bin and workgroup, every thread reading its 32 words.  The
//                                 touched bands are NOT tracked (a tile usually spans one to three): DESIGN section 12 ("Noise curve").
//   noise_curve_resolve_kernel    nine independent workgroups: 0 .. 7 resolve their band with noise_resolve_kernel's scan, 8 sums the eight
//                                 bands per bin first.  No workgroup waits for another; mfill, which needs all rows, is the consumers'.
//   denoise_accumulate_curve_kernel<CH, FIRST, LAST>, denoise_spatial_curve_kernel<CH, S>
//                                 each of the 256 threads forms one entry of the strength table in LDS (noise_curve_entry, noise_curve.hpp: the
//                                 nine rows by uniform loads, validity and mfill in a loop over the eight bands, the interpolation); one
//                                 barrier; then the accumulate's and the top-up's bodies with the divisor's strength replaced by the entry at
//                                 the level of each of the thread's four pixels.  The bodies are the ONE text each that the fixed-strength and
//                                 the auto kernels run, denoise_accumulate_body.hpp and denoise_spatial_body.hpp, included texts that take the
//                                 strength through two macros each.  Every kernel compiles to the code it was
//                                 (profiles/estimated_strength_isa.txt).
#include "denoise.hpp"
#include "denoise_spatial_device.hpp"
#include "image_tile_device.hpp"
#include "noise_curve.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace {

constexpr unsigned kValidBit = 0x01000000u;
static_assert(kNoiseBins == 1024 && kCurveHistWords % kBP == 0, "a key is band << 10 | bin; a thread of the workgroup owns kCurveHistWords / kBP words");
static_assert(kBP == 256, "one thread per entry of the strength table");

// 1 in every byte of w that is 0 or 255
__device__ __forceinline__ unsigned bytes_clipped(unsigned w) { return bytes_zero(w) | bytes_zero(~w); }

__device__ __forceinline__ int byte_at(unsigned w, int c) { return (int)((w >> (8 * c)) & 0xffu); }

// (S + 4) / 9 for S <= 2295 and x / 3 for x <= 766 as multiply-shifts (tests/test_noise_curve_cpu.py proves both exact)
__device__ __forceinline__ unsigned level_of_sum9(unsigned S) { return ((S + 4u) * 7282u) >> 16; }
__device__ __forceinline__ unsigned third(unsigned x) { return (x * 21846u) >> 16; }

// the level of a packed pixel (colour in bytes 0 .. 2): its byte (gray) or (b + g + r + 1) / 3 (BGR)
template <int CH>
__device__ __forceinline__ unsigned curve_level(unsigned packed) {
    if constexpr (CH == 1) return packed & 0xffu;
    return third((packed & 0xffu) + ((packed >> 8) & 0xffu) + ((packed >> 16) & 0xffu) + 1u);
}

// the workgroup's strength table: thread tid forms entry tid; complete behind the caller's barrier
__device__ __forceinline__ void curve_table(unsigned char* s_lut, const unsigned long long* __restrict__ curve36, unsigned scale, unsigned fallback, long long min_samples,
                                            long long band_min_samples) {
    s_lut[threadIdx.x] = (unsigned char)noise_curve_entry(curve36, scale, fallback, min_samples, band_min_samples, (int)threadIdx.x);
}

// the table's entry at the level of the thread's reference pixel j (rw: its packed bytes); >= 1
template <int CH>
__device__ __forceinline__ unsigned curve_strength(const unsigned char* s_lut, const unsigned* rw, int j) {
    unsigned lvl = byte_of(rw, CH * j);
    if constexpr (CH == 3) lvl = third(lvl + byte_of(rw, CH * j + 1) + byte_of(rw, CH * j + 2) + 1u);
    return s_lut[lvl];
}

}  // namespace

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  hist (8 x 1024 words, zeroed by the caller) += the workgroup's banded histogram
template <int CH>
__global__ __launch_bounds__(kBP) void noise_curve_hist_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask, int rows, int cols,
                                                              unsigned* __restrict__ hist) {
    __shared__ __attribute__((aligned(16))) unsigned s_tile[kTileLdsWords];
    __shared__ unsigned s_hist[kCurveHistWords];
    const TileThread t = tile_thread(rows, cols);
    const int nin = t.nin;
    const int64_t p0 = t.p0, npix = (int64_t)rows * cols;

#pragma unroll
    for (int k = 0; k < kCurveHistWords / kBP; ++k) s_hist[t.tid + k * kBP] = 0u;

    unsigned mv = 0u, iw[CH];
#pragma unroll
    for (int d = 0; d < CH; ++d) iw[d] = 0u;
    if (nin) {  // the mask dword first
        unsigned w1[1];
        load_bytes<1>(mask, p0, npix, w1);
        mv = bytes_set(w1[0]) & first_ones(nin);
        if (mv) load_bytes<CH>(image, (int64_t)CH * p0, (int64_t)CH * npix, iw);  // image bytes under an empty mask are not read
    }
    unsigned* own = tile_own(s_tile, t);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned b = kValidBit;
#pragma unroll
        for (int c = 0; c < CH; ++c) b |= byte_of(iw, CH * j + c) << (8 * c);
        own[j] = ((mv >> (8 * j)) & 1u) ? b : 0u;
    }
    if (t.tid < kTileHalo) {
        const TileHalo h = tile_halo(t);
        unsigned b = 0u;
        if (h.hy >= 0 && h.hy < rows && h.hx >= 0 && h.hx < cols) {
            const int64_t p = (int64_t)h.hy * cols + h.hx;
            if (mask[p] != 0) {
                b = kValidBit;
#pragma unroll
                for (int c = 0; c < CH; ++c) b |= (unsigned)image[CH * p + c] << (8 * c);
            }
        }
        s_tile[h.ly * kTileLdsStride + h.lx] = b;
    }
    __syncthreads();

    if (mv) {  // a thread without a set pixel has no candidate
        // the 3 x 6 window, column by column: all three set, any byte clipped, the vertical [1, -2, 1] and [1, 1, 1] per channel
        unsigned all3[6], clip[6];
        int vert[6][CH];
        unsigned vsum[6][CH];
        {
            unsigned win[3][6];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const Lds8* q = static_cast<const Lds8*>(__builtin_assume_aligned(s_tile + (t.ty + r) * kTileLdsStride + 4 * t.g, 8));
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const Lds8 v = q[i];
                    win[r][2 * i] = v[0];
                    win[r][2 * i + 1] = v[1];
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                all3[i] = win[0][i] & win[1][i] & win[2][i];
                clip[i] = bytes_clipped(win[0][i]) | bytes_clipped(win[1][i]) | bytes_clipped(win[2][i]);
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    vert[i][c] = byte_at(win[0][i], c) - 2 * byte_at(win[1][i], c) + byte_at(win[2][i], c);
                    vsum[i][c] = (unsigned)(byte_at(win[0][i], c) + byte_at(win[1][i], c) + byte_at(win[2][i], c));
                }
            }
        }
        constexpr int N = 4 * CH;
        unsigned key[N];
        bool ok[N];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool cand = (all3[j] & all3[j + 1] & all3[j + 2] & kValidBit) != 0u;  // outside the frame and the thread's pixels past nin: 0
            const unsigned cl = clip[j] | clip[j + 1] | clip[j + 2];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int r = vert[j][c] - 2 * vert[j + 1][c] + vert[j + 2][c];
                const unsigned a = (unsigned)(r < 0 ? -r : r);
                const unsigned bin = a > (unsigned)(kNoiseBins - 1) ? (unsigned)(kNoiseBins - 1) : a;
                const unsigned L = level_of_sum9(vsum[j][c] + vsum[j + 1][c] + vsum[j + 2][c]);  // <= 255: the band is 0 .. 7 whatever the bytes
                key[CH * j + c] = ((L >> 5) << 10) | bin;
                ok[CH * j + c] = cand && ((cl >> (8 * c)) & 1u) == 0u;
            }
        }
        // equal keys combined: entry i goes out when no earlier entry has its key, with the count of the entries from i on that have it
#pragma unroll
        for (int i = 0; i < N; ++i) {
            bool lead = ok[i];
            unsigned cnt = 0u;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const bool same = ok[k] && key[k] == key[i];
                if (k < i) lead = lead && !same;
                if (k >= i) cnt += same ? 1u : 0u;
            }
            if (lead) atomicAdd(&s_hist[key[i]], cnt);
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < kCurveHistWords / kBP; ++k) {
        const unsigned v = s_hist[t.tid + k * kBP];
        if (v) atomicAdd(hist + t.tid + k * kBP, v);
    }
}

// grid kCurveRows, block kBP.  Workgroup b < 8: curve[4 b .. 4 b + 3] = the record of hist[b]; workgroup 8: the record of the bands' sum.
// quantile in 1 .. 256
__global__ __launch_bounds__(kBP) void noise_curve_resolve_kernel(const unsigned* __restrict__ hist, unsigned quantile, unsigned long long* __restrict__ curve) {
    constexpr int PER = kNoiseBins / kBP;  // 4 consecutive bins per thread
    __shared__ unsigned s_scan[2][kBP];
    __shared__ unsigned s_m;
    const int tid = (int)threadIdx.x;
    const int row = (int)blockIdx.x;  // (uniform)
    unsigned h[PER], sum = 0u;
#pragma unroll
    for (int i = 0; i < PER; ++i) h[i] = 0u;
    if (row < kCurveBands) {
#pragma unroll
        for (int i = 0; i < PER; ++i) h[i] = hist[row * kNoiseBins + PER * tid + i];
    } else {
        for (int b = 0; b < kCurveBands; ++b)
#pragma unroll
            for (int i = 0; i < PER; ++i) h[i] += hist[b * kNoiseBins + PER * tid + i];  // all samples: < 2^32
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) sum += h[i];
    if (tid == 0) s_m = 0u;
    s_scan[0][tid] = sum;
    __syncthreads();
    int buf = 0;
#pragma unroll
    for (int off = 1; off < kBP; off <<= 1) {  // Hillis-Steele, double-buffered: one barrier per step
        const unsigned v = s_scan[buf][tid] + (tid >= off ? s_scan[buf][tid - off] : 0u);
        s_scan[buf ^ 1][tid] = v;
        buf ^= 1;
        __syncthreads();
    }
    const unsigned long long n = s_scan[buf][kBP - 1];
    const unsigned long long kq = (n * quantile + 255ull) >> 8, k = kq < 1ull ? 1ull : kq;
    const unsigned long long incl = s_scan[buf][tid];
    unsigned long long cum = incl - sum;
    if (n != 0ull && cum < k && k <= incl) {  // exactly one thread
        unsigned m = 0u;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const bool before = cum < k;
            cum += h[i];
            if (before && cum >= k) m = (unsigned)(PER * tid + i);
        }
        s_m = m;
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned long long m = s_m;
        unsigned long long* record = curve + 4 * row;
        record[0] = n;
        record[1] = m;
        record[2] = (256000ull * m + 2023ull) / 4047ull;
        record[3] = 0ull;
    }
}

// denoise_accumulate_auto_kernel's arguments (noise_kernels.hip) with the curve in the record's place and band_min_samples behind min_samples:
// denoise_accumulate_body.hpp's text with the strength of pixel j from the table, where the other two kernels have the launch's one
template <int CH, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBP) void denoise_accumulate_curve_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                                      const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows,
                                                                      int cols, const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode,
                                                                      unsigned fallback, const unsigned long long* __restrict__ curve36, unsigned scale,
                                                                      long long min_samples, long long band_min_samples, unsigned short* __restrict__ cells,
                                                                      unsigned char* __restrict__ out, unsigned char* __restrict__ mask_out,
                                                                      unsigned char* __restrict__ weight, unsigned long long* __restrict__ counts) {
    __shared__ unsigned char s_lut[256];
#define RSDSFM_ACCUMULATE_TABLE curve_table(s_lut, curve36, scale, fallback, min_samples, band_min_samples);
#define RSDSFM_ACCUMULATE_STRENGTH(j) curve_strength<CH>(s_lut, rw, j)
#include "denoise_accumulate_body.hpp"
}

// denoise_spatial_auto_kernel's arguments (noise_kernels.hip) in the same way
template <int CH, int S>
__global__ __launch_bounds__(kBP) void denoise_spatial_curve_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask,
                                                                   const unsigned char* __restrict__ weight, int rows, int cols, unsigned fallback,
                                                                   const unsigned long long* __restrict__ curve36, unsigned scale, long long min_samples,
                                                                   long long band_min_samples, unsigned target, unsigned char* __restrict__ out,
                                                                   unsigned char* __restrict__ support, unsigned long long* __restrict__ counts) {
    __shared__ unsigned char s_lut[256];
    curve_table(s_lut, curve36, scale, fallback, min_samples, band_min_samples);
    __syncthreads();
// the strength at the level of each of the thread's four centre pixels, times CH
#define RSDSFM_SPATIAL_HN_SETUP \
    unsigned hn[4];             \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) hn[j] = (unsigned)s_lut[curve_level<CH>(pk[j])] * (unsigned)CH;
#define RSDSFM_SPATIAL_HN(j) hn[j]
#include "denoise_spatial_body.hpp"
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int noise_curve_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, int channels, int rows, int cols, int quantile, unsigned* d_hist,
                       unsigned long long* d_curve) {
    RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_hist, 0, kCurveHistWords * sizeof(unsigned), c->stream));
    if (channels == 3)
        hipLaunchKernelGGL(noise_curve_hist_kernel<3>, tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_image, d_mask, rows, cols, d_hist);
    else
        hipLaunchKernelGGL(noise_curve_hist_kernel<1>, tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_image, d_mask, rows, cols, d_hist);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    hipLaunchKernelGGL(noise_curve_resolve_kernel, dim3(kCurveRows), dim3(kBP), 0, c->stream, static_cast<const unsigned*>(d_hist), (unsigned)quantile, d_curve);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int denoise_accumulate_curve_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                                    int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int fallback, const unsigned long long* d_curve36,
                                    int scale, int64_t min_samples, int64_t band_min_samples, uint16_t* d_cells, bool first, bool last, unsigned char* d_image_out,
                                    unsigned char* d_mask_out, unsigned char* d_weight, int64_t* d_counts3) {
    if (last && d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, int, int, const unsigned long long*, long long, int,
                            unsigned, const unsigned long long*, unsigned, long long, long long, unsigned short*, unsigned char*, unsigned char*, unsigned char*,
                            unsigned long long*);
    static const Kernel kernels[2][2][2] = {
        {{denoise_accumulate_curve_kernel<1, false, false>, denoise_accumulate_curve_kernel<1, false, true>},
         {denoise_accumulate_curve_kernel<1, true, false>, denoise_accumulate_curve_kernel<1, true, true>}},
        {{denoise_accumulate_curve_kernel<3, false, false>, denoise_accumulate_curve_kernel<3, false, true>},
         {denoise_accumulate_curve_kernel<3, true, false>, denoise_accumulate_curve_kernel<3, true, true>}}};
    // the outputs are passed only to the instances that write them
    hipLaunchKernelGGL(kernels[channels == 3][first][last], tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_ref, d_rmask, d_layer, d_lmask, rows, cols, d_sums,
                       (long long)min_overlap, gain_mode, (unsigned)fallback, d_curve36, (unsigned)scale, (long long)min_samples, (long long)band_min_samples, d_cells,
                       last ? d_image_out : nullptr, last ? d_mask_out : nullptr, last ? d_weight : nullptr,
                       last ? reinterpret_cast<unsigned long long*>(d_counts3) : nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int denoise_spatial_curve_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, const unsigned char* d_weight, int channels, int rows, int cols, int fallback,
                                 const unsigned long long* d_curve36, int scale, int64_t min_samples, int64_t band_min_samples, int target, int search,
                                 unsigned char* d_image_out, unsigned char* d_support, int64_t* d_counts3) {
    if (d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, int, int, unsigned, const unsigned long long*, unsigned, long long, long long,
                            unsigned, unsigned char*, unsigned char*, unsigned long long*);
    static const Kernel kernels[2][3] = {{denoise_spatial_curve_kernel<1, 1>, denoise_spatial_curve_kernel<1, 2>, denoise_spatial_curve_kernel<1, 3>},
                                         {denoise_spatial_curve_kernel<3, 1>, denoise_spatial_curve_kernel<3, 2>, denoise_spatial_curve_kernel<3, 3>}};
    hipLaunchKernelGGL(kernels[channels == 3][search - 1], tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_image, d_mask, d_weight, rows, cols, (unsigned)fallback,
                       d_curve36, (unsigned)scale, (long long)min_samples, (long long)band_min_samples, (unsigned)target, d_image_out, d_support,
                       reinterpret_cast<unsigned long long*>(d_counts3));
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
