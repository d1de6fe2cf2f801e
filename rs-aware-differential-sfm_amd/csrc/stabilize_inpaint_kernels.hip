// stabilize_inpaint_kernels.hip -- the stabiliser's inpainting on MI355X (gfx950, wave64): include/rsdsfm_stabilize_inpaint.h, defined by
// tests/stabilize_inpaint_spec_numpy.py and reproduced bit for bit.  A pull-push pyramid with the structure of the dense rectifier's stage A
// (rectify_dense_kernels.hip) and its level geometry (rectify_dense_plan), for bytes.  Integer arithmetic only; every value goes to memory
// through ordinary stores and one atomicAdd per workgroup.
//
// A cell is ONE 8-byte word, four uint16: [channel 0, channel 1, channel 2, valid (0 or 1)]; an invalid cell is all zero, and a gray image
// leaves channels 1 and 2 zero.  Chosen over a plane per channel because a cell is then one 8-byte load or store, the four children or the
// four taps of a cell are four loads whatever the channel count, the validity costs no plane and no second address, and the three kernels
// between level 1 and the top need no channel template.  The all-zero invalid cell makes the pull branch-free (the fields of the children are
// summed as they are; the valid fields sum to n).  Gray pays 6 unused bytes per cell; the pyramid is 2.7 B per pixel either way and stays
// in the caches between the launches at video sizes.
// The single-workgroup kernel starts at the first level from which everything up to 1 x 1 fits kSmallCells = 8160 cells, the dense
// rectifier's capacity: at 8 bytes per cell that is the same 65280 bytes of LDS, so both pyramids of a frame size split at the same level
// and one plan serves both.
//   inpaint_pull0_kernel<CH>   a thread owns 4 pixels of each of two rows: two level-1 cells.  The mask's and the image's bytes as dwords
//                              where the row's 4 pixels start on one (rows x cols with cols % 4 == 0: always), else byte by byte (and at a
//                              row's last cols % 4 pixels).  Writes level 1 and zeroes the counter.  1 + CH B read per pixel, 2 B written.
//   inpaint_pull_kernel        level l -> l + 1 while the levels are large, a thread per coarser cell.
//   inpaint_small_kernel       ONE workgroup: its lowest level from global memory (or pulled from the level below it), every level above it up
//                              to 1 x 1 and back down in LDS; writes its lowest level complete and the word that says whether the 1 x 1
//                              level is valid.
//   inpaint_push_kernel        fills the invalid cells of level l from the complete level l + 1, down to level 1.
//   inpaint_write_kernel<CH>   grid-stride, 4 consecutive pixels per thread: the mask's dword first; four set bytes and the thread is done, at
//                              1 B read per pixel (the common case).  Else four taps of level 1 per empty pixel, and the image's and the
//                              source's dwords written back merged with what was there.  A thread touches only its own 4 pixels: no race.
//                              It reads the validity word first: a frame without a set pixel is left alone without a host wait.  The
//                              counter as the blend's: a sum per thread, shuffles, LDS, one 64-bit integer atomicAdd per workgroup, only
//                              when a counter was passed.
#include <algorithm>

#include "image_tile_device.hpp"  // bytes_set, bytes_zero, byte_of
#include "rectify_dense.hpp"
#include "rectify_dense_device.hpp"  // kBP, kSB, kSmallCells
#include "rsdsfm_internal.hpp"
#include "stabilize_inpaint.hpp"

namespace rsdsfm {

namespace {

// the sums of a cell's children: s[c] <= 4 x 65280, n = the valid ones
struct CellSum {
    unsigned s0, s1, s2, n;
};

__device__ __forceinline__ void add_cell(CellSum& a, uint2 c) {  // an invalid cell is all zero
    a.s0 += c.x & 0xffffu;
    a.s1 += c.x >> 16;
    a.s2 += c.y & 0xffffu;
    a.n += c.y >> 16;
}

// (s + (n >> 1)) / n for n = 1 .. 4; s (= 0) for n = 0
__device__ __forceinline__ unsigned mean_of(unsigned s, unsigned n) {
    return n == 4u ? (s + 2u) >> 2 : n == 3u ? (s + 1u) / 3u : n == 2u ? (s + 1u) >> 1 : s;
}

__device__ __forceinline__ uint2 cell_of(const CellSum& a) {
    return make_uint2(mean_of(a.s0, a.n) | (mean_of(a.s1, a.n) << 16), mean_of(a.s2, a.n) | ((a.n ? 1u : 0u) << 16));
}

// cell (X, Y) of the level above src (hs x ws)
__device__ __forceinline__ uint2 pull_cells(const uint2* __restrict__ src, int hs, int ws, int X, int Y) {
    const int x0 = 2 * X, y0 = 2 * Y;
    const bool bx = x0 + 1 < ws, by = y0 + 1 < hs;
    const uint2* r0 = src + (int64_t)y0 * ws + x0;
    const uint2 zero = make_uint2(0u, 0u);
    CellSum a = {0u, 0u, 0u, 0u};
    add_cell(a, r0[0]);
    add_cell(a, bx ? r0[1] : zero);
    add_cell(a, by ? r0[ws] : zero);
    add_cell(a, (bx && by) ? r0[ws + 1] : zero);
    return cell_of(a);
}

__device__ __forceinline__ unsigned mix16(unsigned a, unsigned b, unsigned c, unsigned d) { return (9u * a + 3u * b + 3u * c + d + 8u) >> 4; }  // < 2^21 before the shift

// what cell (x, y) of a level takes from the coarser level lv (hc x wc); valid iff lv is (it is complete or all invalid)
__device__ __forceinline__ uint2 push_cells(const uint2* __restrict__ lv, int hc, int wc, int x, int y) {
    const int xn = x >> 1, yn = y >> 1;
    const int xf = min(max(xn + ((x & 1) ? 1 : -1), 0), wc - 1), yf = min(max(yn + ((y & 1) ? 1 : -1), 0), hc - 1);
    const uint2* r0 = lv + (int64_t)yn * wc;
    const uint2* r1 = lv + (int64_t)yf * wc;
    const uint2 a = r0[xn], b = r0[xf], c = r1[xn], d = r1[xf];
    const unsigned v0 = mix16(a.x & 0xffffu, b.x & 0xffffu, c.x & 0xffffu, d.x & 0xffffu);
    const unsigned v1 = mix16(a.x >> 16, b.x >> 16, c.x >> 16, d.x >> 16);
    const unsigned v2 = mix16(a.y & 0xffffu, b.y & 0xffffu, c.y & 0xffffu, d.y & 0xffffu);
    return make_uint2(v0 | (v1 << 16), v2 | (a.y & 0xffff0000u));
}

__device__ __forceinline__ unsigned channel_of(uint2 v, int c) { return c == 0 ? v.x & 0xffffu : c == 1 ? v.x >> 16 : v.y & 0xffffu; }

}  // namespace

// block (64, 4): thread (P, Y) owns pixels 4 P .. 4 P + 3 of rows 2 Y and 2 Y + 1, the level-1 cells (Y, 2 P) and (Y, 2 P + 1)
template <int CH>
__global__ __launch_bounds__(kBP) void inpaint_pull0_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ mask, int rows, int cols,
                                                           uint2* __restrict__ lv1, int h1, int w1, unsigned long long* __restrict__ count) {
    if (count && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) *count = 0ull;  // the output launch adds to it
    const int P = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y;
    const int x0 = 4 * P;
    if (x0 >= cols || Y >= h1) return;
    const int nb = cols - x0 < 4 ? cols - x0 : 4;
    CellSum a[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int y = 2 * Y + r;
        if (y < rows) {
            const int64_t p = (int64_t)y * cols + x0;
            unsigned m = 0u, iw[CH];
#pragma unroll
            for (int d = 0; d < CH; ++d) iw[d] = 0u;
            if (nb == 4 && (p & 3) == 0) {  // the planes are 4-byte aligned: p and CH * p bytes are
                m = *reinterpret_cast<const unsigned*>(mask + p);
#pragma unroll
                for (int d = 0; d < CH; ++d) iw[d] = reinterpret_cast<const unsigned*>(image + CH * p)[d];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nb) {
                        m |= (unsigned)mask[p + j] << (8 * j);
#pragma unroll
                        for (int c = 0; c < CH; ++c) iw[(CH * j + c) >> 2] |= (unsigned)image[CH * (p + j) + c] << (8 * ((CH * j + c) & 3));
                    }
            }
            const unsigned on = bytes_set(m);  // the bytes past nb are 0: absent children
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((on >> (8 * j)) & 1u) {
                    CellSum& t = a[j >> 1];
                    t.n += 1u;
                    t.s0 += byte_of(iw, CH * j) << 8;
                    if (CH == 3) {
                        t.s1 += byte_of(iw, CH * j + 1) << 8;
                        t.s2 += byte_of(iw, CH * j + 2) << 8;
                    }
                }
        }
    }
    uint2* dst = lv1 + (int64_t)Y * w1 + 2 * P;  // 4 P < cols: 2 P < w1
    dst[0] = cell_of(a[0]);
    if (2 * P + 1 < w1) dst[1] = cell_of(a[1]);
}

// block (64, 4), one thread per cell of the coarser level
__global__ __launch_bounds__(kBP) void inpaint_pull_kernel(const uint2* __restrict__ src, int hs, int ws, uint2* __restrict__ dst, int hd, int wd) {
    const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y * 4 + threadIdx.y;
    if (X < wd && Y < hd) dst[(int64_t)Y * wd + X] = pull_cells(src, hs, ws, X, Y);
}

// block (64, 4), one thread per cell of the finer level; valid cells are not touched
__global__ __launch_bounds__(kBP) void inpaint_push_kernel(uint2* __restrict__ lv, int h, int w, const uint2* __restrict__ coarser, int hc, int wc) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const int64_t i = (int64_t)y * w + x;
    if ((lv[i].y >> 16) == 0u) lv[i] = push_cells(coarser, hc, wc, x, y);
}

// ONE workgroup.  Level S (hs x ws; its cells and those of every level above it: at most kSmallCells) comes from `src`: its own incomplete
// cells (reduce_first == 0; src may be dst) or the level below it (hsrc x wsrc), pulled here.  Pull up to 1 x 1 and push back down in LDS;
// dst = level S complete, *top_valid = 1 if the 1 x 1 level is valid (0: the frame has no set pixel).
__global__ __launch_bounds__(kSB) void inpaint_small_kernel(const uint2* src, int hsrc, int wsrc, int reduce_first, int hs, int ws, uint2* dst, unsigned* top_valid) {
    __shared__ uint2 s[kSmallCells];
    __shared__ int s_h[kDenseMaxLevels], s_w[kDenseMaxLevels], s_off[kDenseMaxLevels];
    const int tid = threadIdx.x;
    const int n0 = hs * ws;
    for (int i = tid; i < n0; i += kSB) {
        const int Y = i / ws, X = i - Y * ws;
        s[i] = reduce_first ? pull_cells(src, hsrc, wsrc, X, Y) : src[i];
    }
    int nl = 1, h = hs, w = ws, off = 0;
    if (tid == 0) s_h[0] = hs, s_w[0] = ws, s_off[0] = 0;
    __syncthreads();
    while (h > 1 || w > 1) {  // (uniform)
        const int hn = (h + 1) / 2, wn = (w + 1) / 2, offn = off + h * w;
        for (int i = tid; i < hn * wn; i += kSB) {
            const int Y = i / wn, X = i - Y * wn;
            s[offn + i] = pull_cells(s + off, h, w, X, Y);
        }
        if (tid == 0) s_h[nl] = hn, s_w[nl] = wn, s_off[nl] = offn;
        ++nl;
        h = hn, w = wn, off = offn;
        __syncthreads();
    }
    for (int l = nl - 2; l >= 0; --l) {
        const int hl = s_h[l], wl = s_w[l], ol = s_off[l], hc = s_h[l + 1], wc = s_w[l + 1], oc = s_off[l + 1];
        for (int i = tid; i < hl * wl; i += kSB) {
            const int y = i / wl, x = i - y * wl;
            if ((s[ol + i].y >> 16) == 0u) s[ol + i] = push_cells(s + oc, hc, wc, x, y);
        }
        __syncthreads();
    }
    for (int i = tid; i < n0; i += kSB) dst[i] = s[i];
    if (tid == 0) *top_valid = s[off].y >> 16;
}

// grid-stride over groups of 4 pixels, block kBP: the empty pixels of the image from the complete level 1 (h1 x w1); count += the pixels written
template <int CH>
__global__ __launch_bounds__(kBP) void inpaint_write_kernel(const unsigned char* __restrict__ mask, const uint2* __restrict__ lv1, int h1, int w1,
                                                           const unsigned* __restrict__ top_valid, int rows, int cols, unsigned char* __restrict__ image,
                                                           unsigned char* __restrict__ source, unsigned long long* __restrict__ count) {
    __shared__ unsigned s_wave[kBP / 64];
    if (*top_valid == 0u) return;  // (uniform) no set pixel: nothing is written, and the first launch left the counter 0
    const int npix = rows * cols;  // rows, cols <= 16384
    unsigned nw = 0;               // at most 4 per step and 2^28 / 4 steps in all: no overflow
    const int64_t stride = (int64_t)gridDim.x * kBP * 4;
    for (int64_t q0 = ((int64_t)blockIdx.x * kBP + threadIdx.x) * 4; q0 < npix; q0 += stride) {
        const int p0 = (int)q0;
        if (p0 + 4 <= npix) {  // p0 % 4 == 0: p0 and CH * p0 bytes are 4-byte aligned
            const unsigned empty = bytes_zero(*reinterpret_cast<const unsigned*>(mask + p0));
            if (empty == 0u) continue;  // the common case
            const bool all = empty == 0x01010101u;  // nothing of the 4 pixels is kept: no read
            unsigned* ip = reinterpret_cast<unsigned*>(image + (int64_t)CH * p0);
            unsigned ow[CH];
#pragma unroll
            for (int d = 0; d < CH; ++d) ow[d] = all ? 0u : ip[d];
            int y = p0 / cols, x = p0 - y * cols;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if ((empty >> (8 * j)) & 1u) {
                    const uint2 v = push_cells(lv1, h1, w1, x, y);
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        const int b = CH * j + c, sh = 8 * (b & 3);
                        ow[b >> 2] = (ow[b >> 2] & ~(0xffu << sh)) | (((channel_of(v, c) + 128u) >> 8) << sh);  // <= (65280 + 128) >> 8 = 255
                    }
                }
                if (++x == cols) x = 0, ++y;  // (a group of 4 may span two rows)
            }
#pragma unroll
            for (int d = 0; d < CH; ++d) ip[d] = ow[d];
            if (source) {
                unsigned* sp = reinterpret_cast<unsigned*>(source + p0);
                *sp = all ? 0xffffffffu : (*sp | (empty * kSourceInpainted));  // 255 sets every bit of its byte
            }
            nw += __popc(empty);
        } else {
            for (int p = p0; p < npix; ++p) {
                if (mask[p] != 0) continue;
                const int y = p / cols, x = p - y * cols;
                const uint2 v = push_cells(lv1, h1, w1, x, y);
#pragma unroll
                for (int c = 0; c < CH; ++c) image[(int64_t)CH * p + c] = (unsigned char)((channel_of(v, c) + 128u) >> 8);
                if (source) source[p] = (unsigned char)kSourceInpainted;
                nw += 1u;
            }
        }
    }
    if (!count) return;  // (uniform)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nw += __shfl_down(nw, off, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x / 64] = nw;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kBP / 64; ++w) total += s_wave[w];
        if (total) atomicAdd(count, (unsigned long long)total);
    }
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int inpaint_launch_count(int rows, int cols) {
    const DensePlan p = rectify_dense_plan(rows, cols);
    return p.small == 0 ? 3 : 1 + (p.small - 1) + 1 + p.small + 1;
}

int inpaint_launch(Ctx* c, void* d_pyr, unsigned char* d_image, const unsigned char* d_mask, int channels, int rows, int cols, unsigned char* d_source,
                   int64_t* d_count) {
    const DensePlan p = rectify_dense_plan(rows, cols);
    uint2* pyr = static_cast<uint2*>(d_pyr);
    unsigned* top_valid = reinterpret_cast<unsigned*>(pyr + p.total);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(d_count);
    const auto cells = [](int h, int w) { return dim3((w + 63) / 64, (h + 3) / 4); };
    hipLaunchKernelGGL(channels == 3 ? inpaint_pull0_kernel<3> : inpaint_pull0_kernel<1>, cells(p.h[0], (cols + 3) / 4), dim3(64, 4), 0, c->stream, d_image, d_mask, rows,
                       cols, pyr, p.h[0], p.w[0], cnt);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    const int S = p.small;
    for (int l = 1; l < S; ++l) {  // levels below the single-workgroup launch's source
        hipLaunchKernelGGL(inpaint_pull_kernel, cells(p.h[l], p.w[l]), dim3(64, 4), 0, c->stream, pyr + p.off[l - 1], p.h[l - 1], p.w[l - 1], pyr + p.off[l], p.h[l],
                           p.w[l]);
        RSDSFM_HIP_CHECK(c, hipGetLastError());
    }
    if (S == 0)
        hipLaunchKernelGGL(inpaint_small_kernel, dim3(1), dim3(kSB), 0, c->stream, pyr, 0, 0, 0, p.h[0], p.w[0], pyr, top_valid);
    else
        hipLaunchKernelGGL(inpaint_small_kernel, dim3(1), dim3(kSB), 0, c->stream, pyr + p.off[S - 1], p.h[S - 1], p.w[S - 1], 1, p.h[S], p.w[S], pyr + p.off[S],
                           top_valid);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    for (int l = S - 1; l >= 0; --l) {
        hipLaunchKernelGGL(inpaint_push_kernel, cells(p.h[l], p.w[l]), dim3(64, 4), 0, c->stream, pyr + p.off[l], p.h[l], p.w[l], pyr + p.off[l + 1], p.h[l + 1],
                           p.w[l + 1]);
        RSDSFM_HIP_CHECK(c, hipGetLastError());
    }
    const int64_t nb = ((int64_t)rows * cols + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    hipLaunchKernelGGL(channels == 3 ? inpaint_write_kernel<3> : inpaint_write_kernel<1>, dim3((unsigned)std::min<int64_t>(nb, 65536)), dim3(kBP), 0, c->stream, d_mask,
                       pyr, p.h[0], p.w[0], top_valid, rows, cols, d_image, d_source, cnt);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
