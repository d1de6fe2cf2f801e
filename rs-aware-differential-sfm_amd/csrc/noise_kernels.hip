// noise_kernels.hip -- the noise level on MI355X (gfx950, wave64): include/rsdsfm_noise.h, defined by tests/noise_spec_numpy.py and reproduced
// bit for bit.  Integer arithmetic only; every value goes to memory through ordinary stores and atomicAdd.
//   noise_hist_kernel<CH>       on the 16 x 64 tile of image_tile_device.hpp (the plane reads and the LDS layout with its bank argument are
//                               described there).
//                               Fill: the mask dword first, the image's CH dwords only where a mask byte is set; the packed pixel -- colour in
//                                 bytes 0 .. 2, 1 in byte 3 where the mask is set -- goes to the 18 x 66 LDS plane, 0 for a pixel outside the
//                                 frame, so a frame-border pixel never samples.  The halo byte by byte, mask first.
//                               Window: nine 8-byte reads give the thread's 3 x 6 window.  Per column the AND of the three dwords (byte 3:
//                                 all three set), the OR of their clipped-byte flags (a byte that is 0 or 255, found for four bytes at once) and
//                                 per channel the vertical [1, -2, 1]; per pixel the AND / OR of three columns and the horizontal [1, -2, 1]:
//                                 K is separable.  |r| <= 2024, the bin min(|r|, 1023).
//                               Histogram: 1024 uint32 in LDS (4 KB beside the plane's 4 752 B).  A thread holds at most 4 CH samples; equal
//                                 bins among them are combined in registers and go out as ONE atomicAdd with their count, so a flat frame --
//                                 every sample of the workgroup in bin 0 -- costs one LDS atomic per thread, not twelve.  On a noisy frame
//                                 the samples of a wave spread over some tens of bins.  DESIGN section 12 ("Noise level") has the argument.
//                               Flush: one global 32-bit atomicAdd per non-zero bin and workgroup (a workgroup holds at most 3 072 samples).
//   noise_resolve_kernel        one workgroup: a thread sums four consecutive bins, an inclusive scan of the 256 sums through LDS, the thread
//                               whose range crosses k = max(1, (n q + 255) >> 8) (n q in 64 bits) finds m; thread 0 stores the four words.
//   denoise_accumulate_auto_kernel<CH, FIRST, LAST>, denoise_spatial_auto_kernel<CH, S>
//                               the accumulate's and the top-up's bodies (denoise_device.hpp, a __forceinline__ function as it was in
//                               denoise_kernels.hip; denoise_spatial_body.hpp, an included text, which keeps denoise_spatial_kernel the code it
//                               was) behind two 8-byte loads of the record and the strength's few integer operations, uniform over the launch.
#include "denoise.hpp"
#include "denoise_device.hpp"
#include "denoise_spatial_device.hpp"
#include "image_tile_device.hpp"
#include "noise.hpp"
#include "noise_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace {

constexpr unsigned kValidBit = 0x01000000u;
static_assert(kNoiseBins % kBP == 0, "a thread of the workgroup owns kNoiseBins / kBP bins");

// 1 in every byte of w that is 0 or 255
__device__ __forceinline__ unsigned bytes_clipped(unsigned w) { return bytes_zero(w) | bytes_zero(~w); }

__device__ __forceinline__ int byte_at(unsigned w, int c) { return (int)((w >> (8 * c)) & 0xffu); }

}  // namespace

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  hist (1024 words, zeroed by the caller) += the workgroup's histogram
template <int CH>
__global__ __launch_bounds__(kBP) void noise_hist_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask, int rows, int cols,
                                                        unsigned* __restrict__ hist) {
    __shared__ __attribute__((aligned(16))) unsigned s_tile[kTileLdsWords];
    __shared__ unsigned s_hist[kNoiseBins];
    const TileThread t = tile_thread(rows, cols);
    const int nin = t.nin;
    const int64_t p0 = t.p0, npix = (int64_t)rows * cols;

#pragma unroll
    for (int k = 0; k < kNoiseBins / kBP; ++k) s_hist[t.tid + k * kBP] = 0u;

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
        // the 3 x 6 window, column by column: all three set, any byte clipped, the vertical [1, -2, 1] per channel
        unsigned all3[6], clip[6];
        int vert[6][CH];
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
                for (int c = 0; c < CH; ++c) vert[i][c] = byte_at(win[0][i], c) - 2 * byte_at(win[1][i], c) + byte_at(win[2][i], c);
            }
        }
        constexpr int N = 4 * CH;
        unsigned bin[N];
        bool ok[N];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool cand = (all3[j] & all3[j + 1] & all3[j + 2] & kValidBit) != 0u;  // outside the frame and the thread's pixels past nin: 0
            const unsigned cl = clip[j] | clip[j + 1] | clip[j + 2];
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const int r = vert[j][c] - 2 * vert[j + 1][c] + vert[j + 2][c];
                const unsigned a = (unsigned)(r < 0 ? -r : r);
                bin[CH * j + c] = a > (unsigned)(kNoiseBins - 1) ? (unsigned)(kNoiseBins - 1) : a;
                ok[CH * j + c] = cand && ((cl >> (8 * c)) & 1u) == 0u;
            }
        }
        // equal bins combined: entry i goes out when no earlier entry has its bin, with the count of the entries from i on that have it
#pragma unroll
        for (int i = 0; i < N; ++i) {
            bool lead = ok[i];
            unsigned cnt = 0u;
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const bool same = ok[k] && bin[k] == bin[i];
                if (k < i) lead = lead && !same;
                if (k >= i) cnt += same ? 1u : 0u;
            }
            if (lead) atomicAdd(&s_hist[bin[i]], cnt);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kNoiseBins / kBP; ++k) {
        const unsigned v = s_hist[t.tid + k * kBP];
        if (v) atomicAdd(hist + t.tid + k * kBP, v);
    }
}

// one workgroup of kBP threads.  record[0 .. 3] = [n, m, sigma_q8, 0]; quantile in 1 .. 256
__global__ __launch_bounds__(kBP) void noise_resolve_kernel(const unsigned* __restrict__ hist, unsigned quantile, unsigned long long* __restrict__ record) {
    constexpr int PER = kNoiseBins / kBP;  // 4 consecutive bins per thread
    __shared__ unsigned s_scan[2][kBP];
    __shared__ unsigned s_m;
    const int tid = (int)threadIdx.x;
    unsigned h[PER], sum = 0u;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        h[i] = hist[PER * tid + i];
        sum += h[i];  // n < 2^32
    }
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
        record[0] = n;
        record[1] = m;
        record[2] = (256000ull * m + 2023ull) / 4047ull;
        record[3] = 0ull;
    }
}

// denoise_accumulate_kernel's arguments (denoise_kernels.hip) with the noise record, the scale and min_samples behind `fallback`
template <int CH, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBP) void denoise_accumulate_auto_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                                     const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows,
                                                                     int cols, const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode,
                                                                     unsigned fallback, const unsigned long long* __restrict__ noise4, unsigned scale,
                                                                     long long min_samples, unsigned short* __restrict__ cells, unsigned char* __restrict__ out,
                                                                     unsigned char* __restrict__ mask_out, unsigned char* __restrict__ weight,
                                                                     unsigned long long* __restrict__ counts) {
    const unsigned strength = noise_strength_dev(noise4, scale, min_samples, fallback);  // (uniform)
    denoise_accumulate_body<CH, FIRST, LAST>(ref, rmask, layer, lmask, rows, cols, sums, min_overlap, gain_mode, strength, cells, out, mask_out, weight, counts);
}

// denoise_spatial_kernel's arguments (denoise_spatial_kernels.hip) in the same way
template <int CH, int S>
__global__ __launch_bounds__(kBP) void denoise_spatial_auto_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask,
                                                                  const unsigned char* __restrict__ weight, int rows, int cols, unsigned fallback,
                                                                  const unsigned long long* __restrict__ noise4, unsigned scale, long long min_samples,
                                                                  unsigned target, unsigned char* __restrict__ out, unsigned char* __restrict__ support,
                                                                  unsigned long long* __restrict__ counts) {
    const unsigned strength = noise_strength_dev(noise4, scale, min_samples, fallback);  // (uniform)
#define RSDSFM_SPATIAL_HN_SETUP const unsigned hn = strength * (unsigned)CH;
#define RSDSFM_SPATIAL_HN(j) hn
#include "denoise_spatial_body.hpp"
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int noise_level_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, int channels, int rows, int cols, int quantile, unsigned* d_hist,
                       unsigned long long* d_record) {
    RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_hist, 0, kNoiseBins * sizeof(unsigned), c->stream));
    if (channels == 3)
        hipLaunchKernelGGL(noise_hist_kernel<3>, tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_image, d_mask, rows, cols, d_hist);
    else
        hipLaunchKernelGGL(noise_hist_kernel<1>, tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_image, d_mask, rows, cols, d_hist);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    hipLaunchKernelGGL(noise_resolve_kernel, dim3(1), dim3(kBP), 0, c->stream, static_cast<const unsigned*>(d_hist), (unsigned)quantile, d_record);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int denoise_accumulate_auto_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                                   int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int fallback, const unsigned long long* d_noise4,
                                   int scale, int64_t min_samples, uint16_t* d_cells, bool first, bool last, unsigned char* d_image_out, unsigned char* d_mask_out,
                                   unsigned char* d_weight, int64_t* d_counts3) {
    if (last && d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, int, int, const unsigned long long*, long long, int,
                            unsigned, const unsigned long long*, unsigned, long long, unsigned short*, unsigned char*, unsigned char*, unsigned char*, unsigned long long*);
    static const Kernel kernels[2][2][2] = {
        {{denoise_accumulate_auto_kernel<1, false, false>, denoise_accumulate_auto_kernel<1, false, true>},
         {denoise_accumulate_auto_kernel<1, true, false>, denoise_accumulate_auto_kernel<1, true, true>}},
        {{denoise_accumulate_auto_kernel<3, false, false>, denoise_accumulate_auto_kernel<3, false, true>},
         {denoise_accumulate_auto_kernel<3, true, false>, denoise_accumulate_auto_kernel<3, true, true>}}};
    // the outputs are passed only to the instances that write them
    hipLaunchKernelGGL(kernels[channels == 3][first][last], tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_ref, d_rmask, d_layer, d_lmask, rows, cols, d_sums,
                       (long long)min_overlap, gain_mode, (unsigned)fallback, d_noise4, (unsigned)scale, (long long)min_samples, d_cells, last ? d_image_out : nullptr,
                       last ? d_mask_out : nullptr, last ? d_weight : nullptr, last ? reinterpret_cast<unsigned long long*>(d_counts3) : nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int denoise_spatial_auto_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_mask, const unsigned char* d_weight, int channels, int rows, int cols, int fallback,
                                const unsigned long long* d_noise4, int scale, int64_t min_samples, int target, int search, unsigned char* d_image_out,
                                unsigned char* d_support, int64_t* d_counts3) {
    if (d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, int, int, unsigned, const unsigned long long*, unsigned, long long, unsigned,
                            unsigned char*, unsigned char*, unsigned long long*);
    static const Kernel kernels[2][3] = {{denoise_spatial_auto_kernel<1, 1>, denoise_spatial_auto_kernel<1, 2>, denoise_spatial_auto_kernel<1, 3>},
                                         {denoise_spatial_auto_kernel<3, 1>, denoise_spatial_auto_kernel<3, 2>, denoise_spatial_auto_kernel<3, 3>}};
    hipLaunchKernelGGL(kernels[channels == 3][search - 1], tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_image, d_mask, d_weight, rows, cols, (unsigned)fallback, d_noise4,
                       (unsigned)scale, (long long)min_samples, (unsigned)target, d_image_out, d_support, reinterpret_cast<unsigned long long*>(d_counts3));
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
