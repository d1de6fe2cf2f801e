// erase_kernels.hip -- the mover removal on MI355X (gfx950, wave64): include/rsdsfm_erase.h, defined by tests/erase_spec_numpy.py and reproduced
// bit for bit.  Integer arithmetic only; every value goes to memory through ordinary stores and atomicAdd.
//   matte_seed_cols_kernel      grid-stride, a thread owns 4 consecutive pixels: the flag dwords of the rows y - o .. y + o inside the frame,
//                               each compared PACKED with 2 (include_undecided: with 2 and 3 at once, bit 0 masked off), ANDed, written as a
//                               plane of 0 / 1 bytes -- the seeds eroded along the columns.  Rows outside the frame are skipped: they do not
//                               veto.  cols % 4 == 0: every row starts on a dword and the 4 pixels are one dword per row visited; else byte by
//                               byte, the frame's last pixels included.  Memory: 1 B read from DRAM and 1 B written per pixel; the up to 2 o
//                               rows above and below come from the caches.
//   matte_rows_kernel           a workgroup owns 1024 pixels of ONE row: that plane's bytes of the segment and a halo of o + C - 1 <= 29 on each
//                               side go to LDS (outside the row: 1 -- nothing outside the frame vetoes), 1082 bytes at most; behind ONE barrier
//                               the AND over x - o .. x + o of every position of the segment and a halo of C - 1 (outside the row: 0 -- no core
//                               there) goes to a second LDS row, 1076 bytes at most: the core.  Behind a second barrier every thread scans
//                               outwards from each of its 4 pixels with an early exit at the first core pixel: h = min(C, the distance along
//                               the row to the nearest core pixel), at most 2 (C - 1) = 52 LDS bytes per pixel far from a core.  Memory: 1 B
//                               read (the halo adds 58 / 1024 of that) and 1 B written per pixel, a dword where the 4 pixels start on one.
//   matte_cols_kernel           grid-stride, 4 pixels per thread: d = min over |dy| <= C - 1 inside the frame of max(|dy|, h(y + dy, x)) with the
//                               early exit of seam_distance_cols_kernel (once |dy| reaches the largest of the four best no row can improve any),
//                               and the matte byte a = min(C - d, T) (d <= C).  Away from every core h = C everywhere and a thread reads 2 (C - 1)
//                               more rows from the caches; the segment of a clip that holds a mover is small.
//   erase_composite_kernel<CH>  on the 16 x 64 tile of image_tile_device.hpp (tile_thread, load_bytes, store_group, block_counts_add<5>), no LDS
//                               tile: the matte's and the own mask's dwords first, the own image's CH dwords where a mask byte is set, the
//                               plate's mask only where a matte byte of the group under a set own mask byte is not 0, and the plate's image only
//                               where such a byte also has its plate mask set.  Away from movers CH + 2 B in and CH + 1 B out per pixel.  The
//                               division by the uniform T <= 16 is (x * ceil(65536 / T)) >> 16, exact for every x <= 255 T + T / 2
//                               (tests/test_erase_cpu.py checks every T and x).  Every byte of both outputs is written, no preset.
#include <algorithm>

#include "erase.hpp"
#include "image_tile_device.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace {

constexpr int kSeg = kBP * 4;  // pixels of a row one workgroup of the row pass owns

// 1 in every byte of w that is a seed: care = 0xffffffff: the byte is 2; care = 0xfefefefe: the byte is 2 or 3
__device__ __forceinline__ unsigned seed_bytes(unsigned w, unsigned care) { return bytes_zero((w & care) ^ 0x02020202u); }

}  // namespace

// grid-stride over groups of 4 pixels, block kBP: v(y, x) = 1 iff every flag byte of column x in the rows y - o .. y + o inside the frame is a seed
__global__ __launch_bounds__(kBP) void matte_seed_cols_kernel(const unsigned char* __restrict__ flag, int rows, int cols, int o, unsigned care,
                                                             unsigned char* __restrict__ v) {
    const int npix = rows * cols;        // rows, cols <= 16384
    const bool words = (cols & 3) == 0;  // every row starts on a dword and no group of 4 spans two rows; npix % 4 == 0
    const int64_t stride = (int64_t)gridDim.x * kBP * 4;
    for (int64_t q0 = ((int64_t)blockIdx.x * kBP + threadIdx.x) * 4; q0 < npix; q0 += stride) {
        const int p0 = (int)q0;
        if (words) {
            const int y = p0 / cols;
            const int lo = y - o < 0 ? -y : -o, hi = y + o > rows - 1 ? rows - 1 - y : o;
            unsigned acc = 0x01010101u;
            for (int dy = lo; dy <= hi; ++dy) acc &= seed_bytes(*reinterpret_cast<const unsigned*>(flag + p0 + dy * cols), care);
            *reinterpret_cast<unsigned*>(v + p0) = acc;
        } else {
            for (int p = p0; p < p0 + 4 && p < npix; ++p) {
                const int y = p / cols;
                const int lo = y - o < 0 ? -y : -o, hi = y + o > rows - 1 ? rows - 1 - y : o;
                unsigned acc = 1u;
                for (int dy = lo; dy <= hi; ++dy) acc &= seed_bytes((unsigned)flag[p + dy * cols], care);
                v[p] = (unsigned char)(acc & 1u);
            }
        }
    }
}

// grid (ceil(cols / 1024), rows), block kBP: core(y, x) = the AND of v(y, x - o .. x + o) inside the row; h(y, x) = min(C, the distance along
// row y to the nearest core pixel)
__global__ __launch_bounds__(kBP) void matte_rows_kernel(const unsigned char* __restrict__ v, int rows, int cols, int o, int C, unsigned char* __restrict__ h) {
    __shared__ unsigned char s_v[kSeg + 2 * kEraseHaloMax];
    __shared__ unsigned char s_core[kSeg + 2 * (kEraseReachMax - 1)];
    const int y = blockIdx.y, x0 = (int)blockIdx.x * kSeg, reach = C - 1, halo = o + reach;  // o <= kEraseOpenMax, C <= kEraseReachMax
    const int64_t base = (int64_t)y * cols;
    for (int i = threadIdx.x; i < kSeg + 2 * halo; i += kBP) {
        const int x = x0 - halo + i;
        s_v[i] = (x >= 0 && x < cols) ? (v[base + x] != 0 ? 1 : 0) : 1;  // outside the frame nothing vetoes
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSeg + 2 * reach; i += kBP) {  // position x0 - reach + i, at s_v[i + o]
        const int x = x0 - reach + i;
        unsigned all = (x >= 0 && x < cols) ? 1u : 0u;  // outside the frame there is no core
        for (int dx = 0; dx <= 2 * o; ++dx) all &= s_v[i + dx];  // i + dx <= kSeg + 2 reach - 1 + 2 o
        s_core[i] = (unsigned char)all;
    }
    __syncthreads();
    const int xs = x0 + (int)threadIdx.x * 4;
    const int nb = cols - xs < 4 ? cols - xs : 4;
    if (nb <= 0) return;
    unsigned out = 0u;
    for (int j = 0; j < nb; ++j) {
        const int i = reach + (int)threadIdx.x * 4 + j;  // i - d >= 0 and i + d <= kSeg + 2 reach - 1 for d <= reach
        unsigned val = 0u;
        if (!s_core[i]) {
            val = (unsigned)C;
            for (int d = 1; d < C; ++d)
                if (s_core[i - d] || s_core[i + d]) {
                    val = (unsigned)d;
                    break;
                }
        }
        out |= val << (8 * j);
    }
    unsigned char* dst = h + base + xs;
    if (nb == 4 && ((base + xs) & 3) == 0) {  // the planes are 4-byte aligned
        *reinterpret_cast<unsigned*>(dst) = out;
    } else {
        for (int j = 0; j < nb; ++j) dst[j] = (unsigned char)(out >> (8 * j));
    }
}

// grid-stride over groups of 4 pixels, block kBP: d(y, x) = min over |dy| <= C - 1, inside the frame, of max(|dy|, h(y + dy, x));
// matte(y, x) = min(C - d, T)
__global__ __launch_bounds__(kBP) void matte_cols_kernel(const unsigned char* __restrict__ h, int rows, int cols, int C, int T, unsigned char* __restrict__ matte) {
    const int npix = rows * cols;
    const bool words = (cols & 3) == 0;
    const int64_t stride = (int64_t)gridDim.x * kBP * 4;
    for (int64_t q0 = ((int64_t)blockIdx.x * kBP + threadIdx.x) * 4; q0 < npix; q0 += stride) {
        const int p0 = (int)q0;
        if (words) {
            const int y = p0 / cols;
            const unsigned w = *reinterpret_cast<const unsigned*>(h + p0);
            unsigned b[4] = {w & 0xffu, (w >> 8) & 0xffu, (w >> 16) & 0xffu, w >> 24};
            unsigned top = max(max(b[0], b[1]), max(b[2], b[3]));
            for (int dy = 1; dy < C && (unsigned)dy < top; ++dy) {  // max(dy, .) >= dy: no pixel of the 4 can improve any more
                const unsigned far = (unsigned)C * 0x01010101u;
                const unsigned up = y - dy >= 0 ? *reinterpret_cast<const unsigned*>(h + p0 - dy * cols) : far;
                const unsigned dn = y + dy < rows ? *reinterpret_cast<const unsigned*>(h + p0 + dy * cols) : far;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned d = max(min((up >> (8 * j)) & 0xffu, (dn >> (8 * j)) & 0xffu), (unsigned)dy);
                    b[j] = min(b[j], d);
                }
                top = max(max(b[0], b[1]), max(b[2], b[3]));
            }
            unsigned a = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) a |= min((unsigned)C - b[j], (unsigned)T) << (8 * j);  // b <= C
            *reinterpret_cast<unsigned*>(matte + p0) = a;
        } else {
            for (int p = p0; p < p0 + 4 && p < npix; ++p) {
                const int y = p / cols;
                unsigned b = h[p];
                for (int dy = 1; dy < C && (unsigned)dy < b; ++dy) {
                    const unsigned up = y - dy >= 0 ? h[p - dy * cols] : (unsigned)C;
                    const unsigned dn = y + dy < rows ? h[p + dy * cols] : (unsigned)C;
                    b = min(b, max(min(up, dn), (unsigned)dy));
                }
                matte[p] = (unsigned char)min((unsigned)C - b, (unsigned)T);
            }
        }
    }
}

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  out and mask_out are written whole; counts[0 .. 4] (may be NULL) += [unset, kept, replaced,
// feathered, unresolved].  recip = ceil(65536 / T)
template <int CH>
__global__ __launch_bounds__(kBP) void erase_composite_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                             const unsigned char* __restrict__ plate, const unsigned char* __restrict__ pmask,
                                                             const unsigned char* __restrict__ matte, int rows, int cols, unsigned T, unsigned recip,
                                                             unsigned char* __restrict__ out, unsigned char* __restrict__ mask_out, unsigned long long* __restrict__ counts) {
    const TileThread t = tile_thread(rows, cols);
    const int nin = t.nin;
    const int64_t p0 = t.p0, npix = (int64_t)rows * cols;
    // the matte's and the own mask's dwords first; the plate only under a matte byte that is not 0
    unsigned mr = 0u, aw = 0u, mp = 0u, rw[CH], pw[CH];
#pragma unroll
    for (int d = 0; d < CH; ++d) rw[d] = pw[d] = 0u;
    if (nin) {
        unsigned w1[1];
        load_bytes<1>(matte, p0, npix, w1);
        const unsigned araw = w1[0];
        load_bytes<1>(rmask, p0, npix, w1);
        mr = bytes_set(w1[0]) & first_ones(nin);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned a = min((araw >> (8 * j)) & 0xffu, T);  // a matte byte above T counts as T
            aw |= (((mr >> (8 * j)) & 1u) ? a : 0u) << (8 * j);
        }
        if (mr) load_bytes<CH>(ref, (int64_t)CH * p0, (int64_t)CH * npix, rw);  // image bytes under an empty mask are not read
        if (aw) {
            load_bytes<1>(pmask, p0, npix, w1);
            mp = bytes_set(w1[0]) & bytes_set(aw);
            if (mp) load_bytes<CH>(plate, (int64_t)CH * p0, (int64_t)CH * npix, pw);
        }
    }
    unsigned ow[CH], n5[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < CH; ++d) ow[d] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < nin) {
            const bool set = (mr >> (8 * j)) & 1u, use = (mp >> (8 * j)) & 1u;
            const unsigned a = (aw >> (8 * j)) & 0xffu;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const unsigned r = byte_of(rw, CH * j + c);
                unsigned val = set ? r : 0u;
                if (use) val = ((a * byte_of(pw, CH * j + c) + (T - a) * r + (T >> 1)) * recip) >> 16;  // at most (255 T + T / 2) 65536: no overflow
                ow[(CH * j + c) >> 2] |= val << (8 * ((CH * j + c) & 3));
            }
            n5[0] += set ? 0u : 1u;
            n5[1] += (set && a == 0u) ? 1u : 0u;
            n5[2] += (use && a == T) ? 1u : 0u;
            n5[3] += (use && a != T) ? 1u : 0u;
            n5[4] += (set && a != 0u && !use) ? 1u : 0u;
        }
    unsigned char* const planes[1] = {mask_out};
    const unsigned words[1] = {mr};
    store_group<CH>(out, ow, planes, words, p0, nin);
    block_counts_add<5>(n5, counts);
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int mover_matte_launch(Ctx* c, const unsigned char* d_flag, int rows, int cols, int open, int grow, int feather, int include_undecided, unsigned char* d_v,
                       unsigned char* d_h, unsigned char* d_matte) {
    const int C = open + grow + feather;
    const int64_t nb = ((int64_t)rows * cols + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    const dim3 stride_grid((unsigned)std::min<int64_t>(nb, 65536));
    hipLaunchKernelGGL(matte_seed_cols_kernel, stride_grid, dim3(kBP), 0, c->stream, d_flag, rows, cols, open, include_undecided ? 0xfefefefeu : 0xffffffffu, d_v);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    hipLaunchKernelGGL(matte_rows_kernel, dim3((unsigned)((cols + kSeg - 1) / kSeg), (unsigned)rows), dim3(kBP), 0, c->stream, d_v, rows, cols, open, C, d_h);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    hipLaunchKernelGGL(matte_cols_kernel, stride_grid, dim3(kBP), 0, c->stream, d_h, rows, cols, C, feather, d_matte);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int erase_composite_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_plate, const unsigned char* d_pmask,
                           const unsigned char* d_matte, int channels, int rows, int cols, int feather, unsigned char* d_out, unsigned char* d_mask_out, int64_t* d_counts5) {
    if (d_counts5) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts5, 0, 5 * sizeof(int64_t), c->stream));
    const unsigned T = (unsigned)feather, recip = (65536u + T - 1u) / T;
    hipLaunchKernelGGL(channels == 3 ? erase_composite_kernel<3> : erase_composite_kernel<1>, tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_ref, d_rmask, d_plate, d_pmask,
                       d_matte, rows, cols, T, recip, d_out, d_mask_out, reinterpret_cast<unsigned long long*>(d_counts5));
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
