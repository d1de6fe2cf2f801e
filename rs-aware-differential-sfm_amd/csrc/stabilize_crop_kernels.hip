// stabilize_crop_kernels.hip -- the stabiliser's crop and zoom on MI355X (gfx950): include/rsdsfm_stabilize_crop.h, defined by
// tests/stabilize_crop_spec_numpy.py and reproduced bit for bit.  The window's three kernels are integer arithmetic only:
//   crop_rowscan_kernel   one workgroup per row (and one that zeroes the table's row 0): the planes read as dwords (bytes where the row does
//                         not start on a dword or ends inside one), byte-wise "non-zero" ANDed over the planes, the inclusive prefix count of
//                         the empties along the row -- per thread, wave shuffles, LDS, a carry from tile to tile of 1024 columns -- written as
//                         uint32 into row r + 1 of the (rows + 1) x (cols + 1) table, whose column 0 is zero.  Counts reach 2^28: 32 bits.
//   crop_colscan_kernel   the sums down the columns, in place: a workgroup owns 64 columns (one wave across them: coalesced) and 8 row
//                         segments; every thread sums its segment, LDS gives the segments' offsets, a second walk writes.  Integer sums:
//                         the blocking does not change the table.
//   crop_search_kernel    one anchor per lane, grid-stride: the upper bound min(rows - r, largest h with c + w(h) <= cols), a binary search
//                         over h with 4 table loads per step, the result packed into a 64-bit key whose maximum is the answer; wave
//                         shuffles, LDS, one 64-bit integer atomicMax per workgroup: exact and independent of scheduling.
// and one frame through a window (float64, one rounding per operation, -ffp-contract=off):
//   stabilize_window_warp_kernel / stabilize_window_warp_gray_kernel (3 / 1 channels)
//                         fill_warp_body's structure (stabilize_fill_kernels.hip) -- 4 pixels per thread, the mask's dword first, merged
//                         write-back, byte tail -- with a pixel function that takes the TARGET as two doubles: p = t, p <- t - D(p).  The
//                         window's scalars and the two scale factors are uniform kernel arguments.  Stages A and B are the existing launches.
#include <algorithm>

#include "image_tile_device.hpp"  // bytes_set
#include "rectify_dense.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_crop.hpp"
#include "stabilize_window_device.hpp"

namespace rsdsfm {

namespace {

constexpr int kSegs = 8;  // row segments of the column scan: kCB = 64 columns x 8

// warp_pixel_at, CropMap and window_target: stabilize_window_device.hpp (shared with the occlusion test's warp kernels)
template <int CH>
__device__ __forceinline__ unsigned window_pixel(const unsigned char* __restrict__ img, const float2* __restrict__ disp, int rows, int cols, int iterations,
                                                 const CropMap& wm, int p, unsigned* v) {
    double tx, ty;
    window_target(wm, cols, p, tx, ty);
    return warp_pixel_at<CH>(img, disp, rows, cols, iterations, tx, ty, v);
}

template <int CH>
__device__ __forceinline__ void window_warp_body(const unsigned char* __restrict__ img, const float2* __restrict__ disp, const double* __restrict__ top, int rows,
                                                 int cols, int iterations, unsigned sid, const CropMap wm, unsigned char* __restrict__ out,
                                                 unsigned char* __restrict__ mask, unsigned char* __restrict__ source, unsigned long long* __restrict__ count) {
    __shared__ unsigned s_wave[kBP / 64];
    const int npix = rows * cols;  // rows, cols <= 16384
    unsigned n = 0;                // at most 4 per step and 2^28 / 4 steps in all: no overflow
    if (*top != 0.0) {             // the 1 x 1 level: 0 = the frame has no valid depth = it offers nothing (uniform)
        const int64_t stride = (int64_t)gridDim.x * kBP * 4;
        for (int64_t q0 = ((int64_t)blockIdx.x * kBP + threadIdx.x) * 4; q0 < npix; q0 += stride) {
            const int p0 = (int)q0;
            if (p0 + 4 <= npix) {  // p0 % 4 == 0: p0 and CH * p0 bytes are 4-byte aligned
                unsigned* mw = reinterpret_cast<unsigned*>(mask + p0);
                const unsigned old = *mw;
                if (old == 0x01010101u) continue;
                unsigned v[4 * CH], t[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int c = 0; c < CH; ++c) v[CH * j + c] = 0u;
                    t[j] = 0u;
                    if (((old >> (8 * j)) & 0xffu) == 0u) t[j] = window_pixel<CH>(img, disp, rows, cols, iterations, wm, p0 + j, v + CH * j);
                }
                const unsigned take = t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24);  // 1 in the bytes of the pixels taken
                if (take == 0u) continue;
                n += __popc(take);
                unsigned* dst = reinterpret_cast<unsigned*>(out + (int64_t)CH * p0);
                if (take == 0x01010101u) {  // nothing of the 4 pixels is kept: no read
#pragma unroll
                    for (int d = 0; d < CH; ++d) dst[d] = v[4 * d] | (v[4 * d + 1] << 8) | (v[4 * d + 2] << 16) | (v[4 * d + 3] << 24);
                    if (source) *reinterpret_cast<unsigned*>(source + p0) = sid * 0x01010101u;
                } else {  // (v is 0 in the bytes of the pixels not taken)
#pragma unroll
                    for (int d = 0; d < CH; ++d) {
                        const unsigned sel = (t[4 * d / CH] | (t[(4 * d + 1) / CH] << 8) | (t[(4 * d + 2) / CH] << 16) | (t[(4 * d + 3) / CH] << 24)) * 0xffu;
                        dst[d] = (dst[d] & ~sel) | (v[4 * d] | (v[4 * d + 1] << 8) | (v[4 * d + 2] << 16) | (v[4 * d + 3] << 24));
                    }
                    if (source) {
                        unsigned* sw = reinterpret_cast<unsigned*>(source + p0);
                        *sw = (*sw & ~(take * 0xffu)) | (take * sid);  // sid <= 255: no carry between the bytes
                    }
                }
                *mw = old | take;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (p0 + j < npix && mask[p0 + j] == 0) {
                        unsigned v[CH];
                        if (window_pixel<CH>(img, disp, rows, cols, iterations, wm, p0 + j, v)) {
#pragma unroll
                            for (int c = 0; c < CH; ++c) out[(int64_t)CH * (p0 + j) + c] = (unsigned char)v[c];
                            mask[p0 + j] = 1;
                            if (source) source[p0 + j] = (unsigned char)sid;
                            ++n;
                        }
                    }
            }
        }
    }
    if (!count) return;  // (uniform)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x / 64] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = 0;
#pragma unroll
        for (int w = 0; w < kBP / 64; ++w) total += s_wave[w];
        if (total) atomicAdd(count, (unsigned long long)total);
    }
}

}  // namespace

// grid rows + 1, block kBP.  Block `rows` zeroes the table's row 0; block r writes row r + 1: column 0 zero, column x + 1 the number of
// empties of the planes' AND in columns 0 .. x of row r
__global__ __launch_bounds__(kBP) void crop_rowscan_kernel(const unsigned char* const* __restrict__ planes, int nmasks, int rows, int cols,
                                                          unsigned* __restrict__ table) {
    __shared__ unsigned s_wave[kBP / 64];
    const int tw = cols + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x == rows) {
        for (int x = tid; x < tw; x += kBP) table[x] = 0u;
        return;
    }
    const int r = blockIdx.x;
    unsigned* trow = table + (int64_t)(r + 1) * tw;
    if (tid == 0) trow[0] = 0u;
    const int64_t base = (int64_t)r * cols;
    const bool aligned = (base & 3) == 0;  // the planes are 4-byte aligned
    unsigned carry = 0u;
    for (int x0 = 0; x0 < cols; x0 += kBP * 4) {  // (uniform)
        const int x = x0 + tid * 4;
        const int nb = cols - x < 4 ? cols - x : 4;  // <= 0: nothing of this tile
        unsigned set = 0x01010101u;                  // bytes past the row's end stay set: no empties
        if (nb == 4 && aligned) {
            for (int k = 0; k < nmasks; ++k) set &= bytes_set(*reinterpret_cast<const unsigned*>(planes[k] + base + x));
        } else if (nb > 0) {
            for (int k = 0; k < nmasks; ++k) {
                const unsigned char* src = planes[k] + base + x;
                for (int j = 0; j < nb; ++j)
                    if (src[j] == 0) set &= ~(1u << (8 * j));
            }
        }
        const unsigned e = set ^ 0x01010101u;
        const unsigned e0 = e & 1u, e1 = e0 + ((e >> 8) & 1u), e2 = e1 + ((e >> 16) & 1u), e3 = e2 + (e >> 24);
        unsigned inc = e3;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned t = __shfl_up(inc, off, 64);
            if (lane >= off) inc += t;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        unsigned before = carry, total = 0u;
#pragma unroll
        for (int w = 0; w < kBP / 64; ++w) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        const unsigned excl = before + (inc - e3);
        if (nb > 0) trow[1 + x] = excl + e0;
        if (nb > 1) trow[2 + x] = excl + e1;
        if (nb > 2) trow[3 + x] = excl + e2;
        if (nb > 3) trow[4 + x] = excl + e3;
        carry += total;
        __syncthreads();  // s_wave is written again
    }
}

// grid ceil(cols / 64), block kCB = 64 columns x kSegs row segments: rows 1 .. rows of columns 1 .. cols summed downwards in place
__global__ __launch_bounds__(kCB) void crop_colscan_kernel(int rows, int cols, unsigned* __restrict__ table) {
    __shared__ unsigned s_seg[kSegs][64];
    const int tw = cols + 1, lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int x = 1 + (int)blockIdx.x * 64 + lane;
    const int per = (rows + kSegs - 1) / kSegs;
    const int ra = 1 + seg * per, rb = ra + per < rows + 1 ? ra + per : rows + 1;  // this thread's rows [ra, rb)
    unsigned sum = 0u;
    if (x <= cols)
        for (int r = ra; r < rb; ++r) sum += table[(int64_t)r * tw + x];
    s_seg[seg][lane] = sum;
    __syncthreads();
    unsigned acc = 0u;
    for (int s = 0; s < seg; ++s) acc += s_seg[s][lane];
    if (x <= cols)
        for (int r = ra; r < rb; ++r) {
            acc += table[(int64_t)r * tw + x];
            table[(int64_t)r * tw + x] = acc;
        }
}

// grid-stride over the rows x cols anchors, block kBP; *key = max(*key, the best anchor's key)
__global__ __launch_bounds__(kBP) void crop_search_kernel(const unsigned* __restrict__ table, int rows, int cols, unsigned max_empty, int margin,
                                                         unsigned long long* __restrict__ key) {
    __shared__ unsigned long long s_wave[kBP / 64];
    const int tw = cols + 1, npix = rows * cols;  // rows, cols <= 16384
    const int hmin = (rows + cols - 1) / cols;    // the smallest height with a width
    unsigned long long best = 0ull;
    const int64_t stride = (int64_t)gridDim.x * kBP;
    for (int64_t a = (int64_t)blockIdx.x * kBP + threadIdx.x; a < npix; a += stride) {
        const int r = (int)(a / cols), c = (int)a - r * cols;
        const unsigned* t0 = table + (int64_t)r * tw + c;
        if (max_empty == 0u && (t0[tw + 1] - t0[1]) - (t0[tw] - t0[0]) != 0u) continue;  // the anchor's own pixel is empty
        const int by_width = ((cols - c + 1) * rows - 1) / cols;                          // the largest h with c + w(h) <= cols; < 2^31
        int hi = rows - r < by_width ? rows - r : by_width, lo = hmin - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            const int w = (mid * cols) / rows;
            const int r0 = r - margin > 0 ? r - margin : 0, r1 = r + mid + margin < rows ? r + mid + margin : rows;
            const int c0 = c - margin > 0 ? c - margin : 0, c1 = c + w + margin < cols ? c + w + margin : cols;
            const unsigned* a0 = table + (int64_t)r0 * tw;
            const unsigned* a1 = table + (int64_t)r1 * tw;
            const unsigned n = (a1[c1] - a0[c1]) - (a1[c0] - a0[c0]);
            if (n <= max_empty) lo = mid;
            else hi = mid - 1;
        }
        if (lo >= hmin) {
            const int w = (lo * cols) / rows;
            const int dr = 2 * r + lo - rows, dc = 2 * c + w - cols;
            const unsigned dist = (unsigned)(dr < 0 ? -dr : dr) + (unsigned)(dc < 0 ? -dc : dc);
            const unsigned long long k = ((unsigned long long)lo << 45) | ((unsigned long long)(131071u - dist) << 28) |
                                         ((unsigned long long)(16383 - r) << 14) | (unsigned long long)(16383 - c);
            best = k > best ? k : best;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo32 = __shfl_down((unsigned)best, off, 64), hi32 = __shfl_down((unsigned)(best >> 32), off, 64);
        const unsigned long long o = ((unsigned long long)hi32 << 32) | lo32;
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x / 64] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0ull;
#pragma unroll
        for (int w = 0; w < kBP / 64; ++w) m = s_wave[w] > m ? s_wave[w] : m;
        if (m) atomicMax(key, m);
    }
}

// grid-stride over groups of 4 pixels, block kBP: as stabilize_fill_warp_kernel.  r0 / c0 / sy / sx: the window, see CropMap
__global__ __launch_bounds__(kBP) void stabilize_window_warp_kernel(const unsigned char* __restrict__ img, const float2* __restrict__ disp,
                                                                   const double* __restrict__ top, int rows, int cols, int iterations, unsigned sid, double r0,
                                                                   double c0, double sy, double sx, unsigned char* __restrict__ out,
                                                                   unsigned char* __restrict__ mask, unsigned char* __restrict__ source,
                                                                   unsigned long long* __restrict__ count) {
    window_warp_body<3>(img, disp, top, rows, cols, iterations, sid, CropMap{r0, c0, sy, sx}, out, mask, source, count);
}

__global__ __launch_bounds__(kBP) void stabilize_window_warp_gray_kernel(const unsigned char* __restrict__ img, const float2* __restrict__ disp,
                                                                        const double* __restrict__ top, int rows, int cols, int iterations, unsigned sid,
                                                                        double r0, double c0, double sy, double sx, unsigned char* __restrict__ out,
                                                                        unsigned char* __restrict__ mask, unsigned char* __restrict__ source,
                                                                        unsigned long long* __restrict__ count) {
    window_warp_body<1>(img, disp, top, rows, cols, iterations, sid, CropMap{r0, c0, sy, sx}, out, mask, source, count);
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int crop_window_launch(Ctx* c, const CropWs& ws, int nmasks, int rows, int cols, int64_t max_empty, int margin) {
    RSDSFM_HIP_CHECK(c, hipMemsetAsync(ws.d_key, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(crop_rowscan_kernel, dim3((unsigned)rows + 1u), dim3(kBP), 0, c->stream, ws.d_planes, nmasks, rows, cols, ws.d_table);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    hipLaunchKernelGGL(crop_colscan_kernel, dim3((unsigned)((cols + 63) / 64)), dim3(kCB), 0, c->stream, rows, cols, ws.d_table);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    const int64_t nb = ((int64_t)rows * cols + kBP - 1) / kBP;
    hipLaunchKernelGGL(crop_search_kernel, dim3((unsigned)std::min<int64_t>(nb, 8192)), dim3(kBP), 0, c->stream, ws.d_table, rows, cols, (unsigned)max_empty, margin,
                       ws.d_key);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int stabilize_window_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img_n, int channels, const double* d_depth_cm, const double* d_R, const double* d_t,
                            double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp, int source_id,
                            const int32_t window[4], unsigned char* d_out, unsigned char* d_mask, unsigned char* d_source, int64_t* d_filled) {
    const double* top = nullptr;
    const int rc = rectify_dense_launch_fill(c, ws, d_depth_cm, rows, cols, &top);
    if (rc != RSDSFM_OK) return rc;
    const DensePlan p = rectify_dense_plan(rows, cols);
    const dim3 tiles((cols + kTX - 1) / kTX, (rows + kTY - 1) / kTY);
    hipLaunchKernelGGL(stabilize_map_kernel, tiles, dim3(kCB), 0, c->stream, d_depth_cm, ws.d_pyr, p.h[0], p.w[0], d_R, d_t, fx, fy, cx, cy, q5_mode == 0 ? fx : fy, rows,
                       cols, mode, vp, ws.d_disp, (double*)nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    if (d_filled) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_filled, 0, sizeof(int64_t), c->stream));
    const int64_t npix = (int64_t)rows * cols;
    const int64_t nb = (npix + (int64_t)kBP * 4 - 1) / ((int64_t)kBP * 4);
    const double sy = (double)window[2] / (double)rows, sx = (double)window[3] / (double)cols;
    hipLaunchKernelGGL(channels == 3 ? stabilize_window_warp_kernel : stabilize_window_warp_gray_kernel, dim3((unsigned)std::min<int64_t>(nb, 65536)), dim3(kBP), 0,
                       c->stream, d_img_n, ws.d_disp, top, rows, cols, iterations, (unsigned)source_id, (double)window[0], (double)window[1], sy, sx, d_out, d_mask,
                       d_source, reinterpret_cast<unsigned long long*>(d_filled));
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
