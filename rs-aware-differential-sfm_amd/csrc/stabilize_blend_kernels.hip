// stabilize_blend_kernels.hip -- the stabiliser's seam blend on MI355X (gfx950, wave64): include/rsdsfm_stabilize_blend.h, defined by
// tests/stabilize_blend_spec_numpy.py and reproduced bit for bit.  Integer arithmetic only; every value goes to memory through ordinary
// stores and atomicAdd.
//   seam_distance_rows_kernel   a workgroup owns 1024 pixels of ONE row: the "set" bytes of the segment and a halo of T - 1 on each side
//                               (outside the frame: set -- the frame's edge is not a hole) go to LDS, 1150 bytes at most, and every thread
//                               scans outwards from each of its 4 pixels with an early exit at the first empty one: at most 2 (T - 1) LDS
//                               bytes per pixel, 30 at T = 16, far from an empty pixel.  Chosen over a two-sweep scan for its size; the
//                               launch is not bound by it at 720p.  Memory: 1 B read (the halo adds 2 (T - 1) / 1024 of that) and 1 B
//                               written per pixel, as a dword where the row's 4 pixels start on one, else byte by byte (the byte path: rows
//                               whose cols % 4 != 0, and every row's last cols % 4 pixels).
//   seam_distance_cols_kernel   grid-stride, a thread owns 4 consecutive pixels: d = min over |dy| <= T - 1 of max(|dy|, h(y + dy, x)), rows
//                               outside the frame skipped, with an early exit once |dy| reaches the best so far.  cols % 4 == 0: every row
//                               starts on a dword and the 4 pixels are one dword of h per row visited; else byte by byte, the frame's last
//                               pixels included (the byte tail).  Memory: 1 B of h read from DRAM and 1 B written per pixel; the rows above
//                               and below, up to 2 (T - 1) more bytes per pixel where no empty pixel is near, come from the caches (a
//                               workgroup's neighbours in y read the same lines).
//   seam_overlap_sums_kernel<CH>  grid-stride, 4 pixels per thread: the source dword and the layer mask's dword first (2 B per pixel), the
//                               image's and the layer's dwords (2 CH B per pixel) only when some byte has source == 1 under a set layer
//                               mask; 64-bit sums per thread, shuffles, LDS, one 64-bit integer atomicAdd per sum and workgroup: exact and
//                               independent of scheduling.
//   seam_blend_kernel<CH>       the same ownership: the distance dword and the source dword first; all four bytes T and no source byte 0 and
//                               the thread is done, at 2 B read per pixel (the common case, away from the band).  Else the layer mask, then
//                               the layer's and the image's dwords, and the image, mask and source dwords written back merged with what was
//                               there.  A thread touches only its own 4 pixels of the in-out planes: no race.  Every workgroup computes the
//                               gains itself from the 8-word record (CH 64-bit divisions, threads 0 .. CH - 1, through LDS): no host wait
//                               between the sums and the blend.  The two counters as the fill's: a sum per thread, shuffles, LDS, one 64-bit
//                               integer atomicAdd each per workgroup, only when a counter pointer was passed.
#include <algorithm>

#include "image_tile_device.hpp"  // bytes_set, bytes_zero, byte_of
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {

namespace {

constexpr int kSeg = kBP * 4;  // pixels of a row one workgroup of the row pass owns

__device__ __forceinline__ unsigned long long shfl_down64(unsigned long long v, int off) {
    const unsigned lo = __shfl_down((unsigned)v, off, 64), hi = __shfl_down((unsigned)(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}

template <int CH>
__device__ __forceinline__ void overlap_sums_body(const unsigned char* __restrict__ image, const unsigned char* __restrict__ source,
                                                  const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                  unsigned long long* __restrict__ sums, unsigned long long* __restrict__ counts) {
    constexpr int NS = 1 + 2 * CH;
    __shared__ unsigned long long s_part[kBP / 64][NS];
    if (counts && blockIdx.x == 0 && threadIdx.x < 2) counts[threadIdx.x] = 0ull;  // the blend launch behind this one adds to them
    const int npix = rows * cols;  // rows, cols <= 16384
    // 64-bit per thread: a sum is at most 255 x 2^28 < 2^36 over the WHOLE frame, so no thread's share overflows whatever the grid; the
    // count is at most 2^28
    unsigned long long acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) acc[i] = 0ull;
    const int64_t stride = (int64_t)gridDim.x * kBP * 4;
    for (int64_t q0 = ((int64_t)blockIdx.x * kBP + threadIdx.x) * 4; q0 < npix; q0 += stride) {
        const int p0 = (int)q0;
        if (p0 + 4 <= npix) {  // p0 % 4 == 0: p0 and CH * p0 bytes are 4-byte aligned
            const unsigned sw = *reinterpret_cast<const unsigned*>(source + p0);
            const unsigned lm = *reinterpret_cast<const unsigned*>(lmask + p0);
            const unsigned q = bytes_zero(sw ^ 0x01010101u) & bytes_set(lm);
            if (q == 0u) continue;
            unsigned iw[CH], lw[CH];
#pragma unroll
            for (int d = 0; d < CH; ++d) {
                iw[d] = reinterpret_cast<const unsigned*>(image + (int64_t)CH * p0)[d];
                lw[d] = reinterpret_cast<const unsigned*>(layer + (int64_t)CH * p0)[d];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((q >> (8 * j)) & 1u) {
                    acc[0] += 1ull;
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        acc[1 + c] += byte_of(iw, CH * j + c);
                        acc[1 + CH + c] += byte_of(lw, CH * j + c);
                    }
                }
        } else {
            for (int p = p0; p < npix; ++p)
                if (source[p] == 1 && lmask[p] != 0) {
                    acc[0] += 1ull;
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        acc[1 + c] += image[(int64_t)CH * p + c];
                        acc[1 + CH + c] += layer[(int64_t)CH * p + c];
                    }
                }
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[i] += shfl_down64(acc[i], off);
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x / 64][i] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        unsigned long long total = 0ull;
#pragma unroll
        for (int w = 0; w < kBP / 64; ++w) total += s_part[w][threadIdx.x];
        if (total) atomicAdd(sums + threadIdx.x, total);
    }
}

template <int CH>
__device__ __forceinline__ void seam_blend_body(const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask,
                                                const unsigned char* __restrict__ dist, unsigned T, unsigned sid, int rows, int cols,
                                                const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode,
                                                unsigned char* __restrict__ image, unsigned char* __restrict__ mask, unsigned char* __restrict__ source,
                                                unsigned long long* __restrict__ counts) {
    __shared__ unsigned s_gain[CH];
    __shared__ unsigned s_wave[2][kBP / 64];
    if (threadIdx.x < CH) s_gain[threadIdx.x] = seam_gain(sums, CH, threadIdx.x, min_overlap, gain_mode);
    __syncthreads();
    unsigned G[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) G[c] = s_gain[c];
    const int npix = rows * cols;  // rows, cols <= 16384
    const unsigned Tw = T * 0x01010101u, half = T >> 1;
    unsigned nf = 0, nm = 0;  // at most 4 per step and 2^28 / 4 steps in all: no overflow
    const int64_t stride = (int64_t)gridDim.x * kBP * 4;
    for (int64_t q0 = ((int64_t)blockIdx.x * kBP + threadIdx.x) * 4; q0 < npix; q0 += stride) {
        const int p0 = (int)q0;
        if (p0 + 4 <= npix) {  // p0 % 4 == 0: p0 and CH * p0 bytes are 4-byte aligned
            const unsigned dw = *reinterpret_cast<const unsigned*>(dist + p0);
            unsigned* sp = reinterpret_cast<unsigned*>(source + p0);
            const unsigned sw = *sp;
            if (dw == Tw && bytes_set(sw) == 0x01010101u) continue;  // deep inside the own frame or taken already: nothing to do
            const unsigned on = bytes_set(*reinterpret_cast<const unsigned*>(lmask + p0));
            if (on == 0u) continue;
            const unsigned fill = on & bytes_zero(sw);
            unsigned mix = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (((sw >> (8 * j)) & 0xffu) == 1u && ((dw >> (8 * j)) & 0xffu) < T) mix |= 1u << (8 * j);
            mix &= on;
            const unsigned act = fill | mix;
            if (act == 0u) continue;
            unsigned* ip = reinterpret_cast<unsigned*>(image + (int64_t)CH * p0);
            unsigned iw[CH], lw[CH], ow[CH];
#pragma unroll
            for (int d = 0; d < CH; ++d) {
                lw[d] = reinterpret_cast<const unsigned*>(layer + (int64_t)CH * p0)[d];
                iw[d] = fill == 0x01010101u ? 0u : ip[d];  // nothing of the 4 pixels is kept: no read
                ow[d] = 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned dj = (dw >> (8 * j)) & 0xffu;
                const bool f = (fill >> (8 * j)) & 1u, m = (mix >> (8 * j)) & 1u;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int b = CH * j + c;
                    const unsigned own = byte_of(iw, b);
                    const unsigned k = gained(G[c], byte_of(lw, b));
                    const unsigned v = f ? k : m ? (dj * own + (T - dj) * k + half) / T : own;  // dj < T where m: <= 255
                    ow[b >> 2] |= v << (8 * (b & 3));
                }
            }
#pragma unroll
            for (int d = 0; d < CH; ++d) ip[d] = ow[d];
            if (fill) {
                unsigned* mp = reinterpret_cast<unsigned*>(mask + p0);
                *mp = (*mp & ~(fill * 0xffu)) | fill;
            }
            *sp = (sw & ~(act * 0xffu)) | (act * sid);  // sid <= 255: no carry between the bytes
            nf += __popc(fill);
            nm += __popc(mix);
        } else {
            for (int p = p0; p < npix; ++p) {
                if (lmask[p] == 0) continue;
                const unsigned s = source[p], dj = dist[p];
                const bool f = s == 0u, m = s == 1u && dj < T;
                if (!f && !m) continue;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const unsigned k = gained(G[c], layer[(int64_t)CH * p + c]);
                    const unsigned own = image[(int64_t)CH * p + c];
                    image[(int64_t)CH * p + c] = (unsigned char)(f ? k : (dj * own + (T - dj) * k + half) / T);
                }
                if (f) mask[p] = 1;
                source[p] = (unsigned char)sid;
                nf += f ? 1u : 0u;
                nm += f ? 0u : 1u;
            }
        }
    }
    if (!counts) return;  // (uniform)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nf += __shfl_down(nf, off, 64);
        nm += __shfl_down(nm, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_wave[0][threadIdx.x / 64] = nf;
        s_wave[1][threadIdx.x / 64] = nm;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kBP / 64; ++w) total += s_wave[threadIdx.x][w];
        if (total) atomicAdd(counts + threadIdx.x, (unsigned long long)total);
    }
}

}  // namespace

// grid (ceil(cols / 1024), rows), block kBP: h(y, x) = min(T, the distance along row y to the nearest pixel whose mask byte is 0)
__global__ __launch_bounds__(kBP) void seam_distance_rows_kernel(const unsigned char* __restrict__ mask, int rows, int cols, int T, unsigned char* __restrict__ h) {
    __shared__ unsigned char s_set[kSeg + 2 * (kFeatherMax - 1)];
    const int y = blockIdx.y, x0 = (int)blockIdx.x * kSeg, halo = T - 1;  // T <= kFeatherMax
    const int64_t base = (int64_t)y * cols;
    for (int i = threadIdx.x; i < kSeg + 2 * halo; i += kBP) {
        const int x = x0 - halo + i;
        s_set[i] = (x >= 0 && x < cols) ? (mask[base + x] != 0 ? 1 : 0) : 1;
    }
    __syncthreads();
    const int xs = x0 + (int)threadIdx.x * 4;
    const int nb = cols - xs < 4 ? cols - xs : 4;
    if (nb <= 0) return;
    unsigned out = 0u;
    for (int j = 0; j < nb; ++j) {
        const int i = halo + (int)threadIdx.x * 4 + j;  // i - d >= 0 and i + d <= kSeg + 2 halo - 1 for d <= halo
        unsigned v = 0u;
        if (s_set[i]) {
            v = (unsigned)T;
            for (int d = 1; d < T; ++d)
                if (!s_set[i - d] || !s_set[i + d]) {
                    v = (unsigned)d;
                    break;
                }
        }
        out |= v << (8 * j);
    }
    unsigned char* dst = h + base + xs;
    if (nb == 4 && ((base + xs) & 3) == 0) {  // the planes are 4-byte aligned
        *reinterpret_cast<unsigned*>(dst) = out;
    } else {
        for (int j = 0; j < nb; ++j) dst[j] = (unsigned char)(out >> (8 * j));
    }
}

// grid-stride over groups of 4 pixels, block kBP: d(y, x) = min over |dy| <= T - 1, inside the frame, of max(|dy|, h(y + dy, x))
__global__ __launch_bounds__(kBP) void seam_distance_cols_kernel(const unsigned char* __restrict__ h, int rows, int cols, int T, unsigned char* __restrict__ dist) {
    const int npix = rows * cols;  // rows, cols <= 16384
    const bool words = (cols & 3) == 0;  // every row starts on a dword and no group of 4 spans two rows; npix % 4 == 0
    const int64_t stride = (int64_t)gridDim.x * kBP * 4;
    for (int64_t q0 = ((int64_t)blockIdx.x * kBP + threadIdx.x) * 4; q0 < npix; q0 += stride) {
        const int p0 = (int)q0;
        if (words) {
            const int y = p0 / cols;
            const unsigned w = *reinterpret_cast<const unsigned*>(h + p0);
            unsigned b[4] = {w & 0xffu, (w >> 8) & 0xffu, (w >> 16) & 0xffu, w >> 24};
            unsigned top = max(max(b[0], b[1]), max(b[2], b[3]));
            for (int dy = 1; dy < T && (unsigned)dy < top; ++dy) {  // max(dy, .) >= dy: no pixel of the 4 can improve any more
                const unsigned far = (unsigned)T * 0x01010101u;
                const unsigned up = y - dy >= 0 ? *reinterpret_cast<const unsigned*>(h + p0 - dy * cols) : far;
                const unsigned dn = y + dy < rows ? *reinterpret_cast<const unsigned*>(h + p0 + dy * cols) : far;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned v = max(min((up >> (8 * j)) & 0xffu, (dn >> (8 * j)) & 0xffu), (unsigned)dy);
                    b[j] = min(b[j], v);
                }
                top = max(max(b[0], b[1]), max(b[2], b[3]));
            }
            *reinterpret_cast<unsigned*>(dist + p0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        } else {
            for (int p = p0; p < p0 + 4 && p < npix; ++p) {
                const int y = p / cols;
                unsigned b = h[p];
                for (int dy = 1; dy < T && (unsigned)dy < b; ++dy) {
                    const unsigned up = y - dy >= 0 ? h[p - dy * cols] : (unsigned)T;
                    const unsigned dn = y + dy < rows ? h[p + dy * cols] : (unsigned)T;
                    b = min(b, max(min(up, dn), (unsigned)dy));
                }
                dist[p] = (unsigned char)b;
            }
        }
    }
}

// grid-stride over groups of 4 pixels, block kBP: sums[0 .. 2 CH] += [count, sum image_c, sum layer_c] over source == 1 under a set layer mask
template <int CH>
__global__ __launch_bounds__(kBP) void seam_overlap_sums_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ source,
                                                               const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                               unsigned long long* __restrict__ sums, unsigned long long* __restrict__ counts) {
    overlap_sums_body<CH>(image, source, layer, lmask, rows, cols, sums, counts);
}

// grid-stride over groups of 4 pixels, block kBP: image, mask and source are in-out; counts[0] += filled, counts[1] += blended
template <int CH>
__global__ __launch_bounds__(kBP) void seam_blend_kernel(const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask,
                                                        const unsigned char* __restrict__ dist, unsigned T, unsigned sid, int rows, int cols,
                                                        const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode,
                                                        unsigned char* __restrict__ image, unsigned char* __restrict__ mask, unsigned char* __restrict__ source,
                                                        unsigned long long* __restrict__ counts) {
    seam_blend_body<CH>(layer, lmask, dist, T, sid, rows, cols, sums, min_overlap, gain_mode, image, mask, source, counts);
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int seam_distance_launch(Ctx* c, const unsigned char* d_mask, int rows, int cols, int feather, unsigned char* d_h, unsigned char* d_dist) {
    hipLaunchKernelGGL(seam_distance_rows_kernel, dim3((unsigned)((cols + kSeg - 1) / kSeg), (unsigned)rows), dim3(kBP), 0, c->stream, d_mask, rows, cols, feather, d_h);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    const int64_t nb = ((int64_t)rows * cols + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    hipLaunchKernelGGL(seam_distance_cols_kernel, dim3((unsigned)std::min<int64_t>(nb, 65536)), dim3(kBP), 0, c->stream, d_h, rows, cols, feather, d_dist);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int seam_overlap_sums_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_source, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                             int rows, int cols, unsigned long long* d_sums, unsigned long long* d_counts) {
    RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_sums, 0, 8 * sizeof(unsigned long long), c->stream));
    const int64_t nb = ((int64_t)rows * cols + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    const dim3 grid((unsigned)std::min<int64_t>(nb, 65536));
    hipLaunchKernelGGL(channels == 3 ? seam_overlap_sums_kernel<3> : seam_overlap_sums_kernel<1>, grid, dim3(kBP), 0, c->stream, d_image, d_source, d_layer, d_lmask, rows,
                       cols, d_sums, d_counts);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int seam_blend_launch(Ctx* c, const unsigned char* d_layer, const unsigned char* d_lmask, int channels, int rows, int cols, const unsigned char* d_dist, int feather,
                      int64_t min_overlap, int gain_mode, int source_id, unsigned char* d_image, unsigned char* d_mask, unsigned char* d_source,
                      unsigned long long* d_sums, int64_t* d_counts) {
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(d_counts);
    const int rc = seam_overlap_sums_launch(c, d_image, d_source, d_layer, d_lmask, channels, rows, cols, d_sums, cnt);
    if (rc != RSDSFM_OK) return rc;
    const int64_t nb = ((int64_t)rows * cols + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    const dim3 grid((unsigned)std::min<int64_t>(nb, 65536));
    hipLaunchKernelGGL(channels == 3 ? seam_blend_kernel<3> : seam_blend_kernel<1>, grid, dim3(kBP), 0, c->stream, d_layer, d_lmask, d_dist, (unsigned)feather,
                       (unsigned)source_id, rows, cols, d_sums, (long long)min_overlap, gain_mode, d_image, d_mask, d_source, cnt);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
