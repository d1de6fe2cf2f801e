// last_frame_kernels.hip -- a pair's depth map moved onto its second frame's grid on MI355X (gfx950): include/rsdsfm_last_frame.h, defined
// by tests/last_frame_spec_numpy.py and reproduced bit for bit (float64 arithmetic, one rounding per operation, -ffp-contract=off; the
// numbered steps are the link spec's).  The per-pixel expressions are flatten_point's (device_math.hpp), which has no fused form: both
// library builds compile this file the same way.  It is the fusion's splat (fuse_kernels.hip) for one pair with a ratio of exactly 1.0, and
// a resolve that turns the plane into a depth map.
//
//   advance_preset_kernel   the plane to all ones: 16 B per lane, a byte tail of one word for an odd pixel count.
//   advance_splat_kernel    one lane per pixel of the row-major field (16 B per lane with a depth), a 64 x 16 tile of the column-major depth
//                           map through LDS.  It ends in ONE 64-bit unsigned atomicMin of z_pred's bit pattern on the landing pixel.  A
//                           valid depth is a positive finite double, so its pattern orders as an integer: an exact z-buffer that does not
//                           depend on the order of the offers, without a floating atomic.  Workgroup (0, 0) zeroes the counter.
//   advance_resolve_kernel  the row-major plane (8 B per lane, coalesced along x) through the LDS tile into the column-major map (coalesced
//                           along y), +0.0 where the plane kept its preset.  The count: a wave shuffle, an LDS sum over the four waves,
//                           one 64-bit integer atomicAdd per workgroup.
//
// Algorithmic HBM traffic per pixel: 8 B written (preset); 8 B (Z) + 16 B (field) read and one 8 B atomic (splat); 8 B read + 8 B written
// (resolve).  No private segment.
#include <math.h>

#include "device_math.hpp"
#include "last_frame.hpp"

namespace rsdsfm {

namespace {

constexpr int kAB = 256;             // threads of a workgroup: 4 waves
constexpr int kATX = 64, kATY = 16;  // tile: 64 columns x 16 rows, 4 pixels per lane
constexpr unsigned long long kNothing = ~0ull;

__device__ __forceinline__ bool valid_depth(double z) { return z > 0.0 && z < INFINITY; }  // finite and > 0; false for NaN
__device__ __forceinline__ bool usable_vector(double2 f) { return fabs(f.x) < INFINITY && fabs(f.y) < INFINITY && !(f.x == 0.0 && f.y == 0.0); }

}  // namespace

// grid: ceil(ceil(npix / 2) / kAB) workgroups, one ulonglong2 per lane
__global__ __launch_bounds__(kAB) void advance_preset_kernel(unsigned long long* __restrict__ plane, size_t npix) {
    const size_t i = ((size_t)blockIdx.x * kAB + threadIdx.x) * 2;
    if (i + 1 < npix)
        *reinterpret_cast<ulonglong2*>(plane + i) = make_ulonglong2(kNothing, kNothing);  // (the plane is 16-byte aligned: checked by the host)
    else if (i < npix)
        plane[i] = kNothing;
}

// grid: (ceil(cols / kATX), ceil(rows / kATY))
__global__ __launch_bounds__(kAB) void advance_splat_kernel(const double* __restrict__ field, const double* __restrict__ zmap, double v2, double w0, double w1,
                                                            double k, LinkCamera cam, int rows, int cols, unsigned long long* __restrict__ plane,
                                                            unsigned long long* __restrict__ count) {
    __shared__ double s_z[kATX][kATY + 1];
    const int x0 = (int)blockIdx.x * kATX, y0 = (int)blockIdx.y * kATY;
    const int tid = (int)threadIdx.x;
    if (count && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *count = 0ull;  // the resolve, behind this launch, adds to it
    {  // the tile of the column-major map, coalesced along y; 0 outside the frame
        const int ly = tid & (kATY - 1);
#pragma unroll
        for (int j = 0; j < kATX * kATY / kAB; ++j) {
            const int lx = tid / kATY + j * (kAB / kATY);
            const int xx = x0 + lx, yy = y0 + ly;
            s_z[lx][ly] = (xx < cols && yy < rows) ? zmap[(size_t)xx * (size_t)rows + (size_t)yy] : 0.0;
        }
    }
    __syncthreads();
    const int lx = tid & (kATX - 1), x = x0 + lx;
    const int wv = tid / kATX;
    const double h = (double)rows;
#pragma unroll
    for (int j = 0; j < kATY / (kAB / kATX); ++j) {
        const int ly = wv + j * (kAB / kATX);
        const int y = y0 + ly;  // wave-uniform
        if (!(x < cols && y < rows)) continue;
        const double z = s_z[lx][ly];
        if (!valid_depth(z)) continue;
        const size_t idx = (size_t)y * (size_t)cols + (size_t)x;
        const double2 f = *reinterpret_cast<const double2*>(field + 2 * idx);
        if (!usable_vector(f)) continue;
        const FlatPoint p = flatten_point(f, x, y, cam.fx, cam.fy, cam.cx, cam.cy, cam.gamma, h);                    // 1
        const double alpha = cam.global_shutter ? 1.0 : p.alpha;
        const double beta = (2.0 * (alpha + k * p.alpha_k)) / (2.0 + k);                                               // 2
        const double b = beta / cam.gamma;
        const double z_pred = z * (1.0 + b * (w0 * p.qy - w1 * p.qx)) + b * v2;                                        // 3
        const double r2 = floor(((double)y + f.y) + 0.5), c2 = floor(((double)x + f.x) + 0.5);                         // 4
        const bool inside = r2 >= 0.0 && r2 <= (double)(rows - 1) && c2 >= 0.0 && c2 <= (double)(cols - 1);
        if (inside && valid_depth(z_pred))
            atomicMin(&plane[(size_t)(int)r2 * (size_t)cols + (size_t)(int)c2], (unsigned long long)__double_as_longlong(z_pred));  // inside the plane
    }
}

// grid: (ceil(cols / kATX), ceil(rows / kATY))
__global__ __launch_bounds__(kAB) void advance_resolve_kernel(const unsigned long long* __restrict__ plane, int rows, int cols, double* __restrict__ out,
                                                              unsigned long long* __restrict__ count) {
    __shared__ double s_z[kATX][kATY + 1];
    __shared__ int s_count;
    const int x0 = (int)blockIdx.x * kATX, y0 = (int)blockIdx.y * kATY;
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_count = 0;
    __syncthreads();
    const int lx = tid & (kATX - 1), x = x0 + lx;
    const int wv = tid / kATX;
    int n = 0;
#pragma unroll
    for (int j = 0; j < kATY / (kAB / kATX); ++j) {
        const int ly = wv + j * (kAB / kATX);
        const int y = y0 + ly;  // wave-uniform
        double z = 0.0;
        if (x < cols && y < rows) {
            const unsigned long long word = plane[(size_t)y * (size_t)cols + (size_t)x];
            if (word != kNothing) {
                z = __longlong_as_double((long long)word);
                ++n;
            }
        }
        s_z[lx][ly] = z;  // (the lane's own cell)
    }
    if (count) {  // (uniform)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) n += __shfl_down(n, d, 64);
        if ((tid & 63) == 0 && n) atomicAdd(&s_count, n);
    }
    __syncthreads();  // the tile holds the depths, the count is complete
    {
        const int ly = tid & (kATY - 1);
#pragma unroll
        for (int j = 0; j < kATX * kATY / kAB; ++j) {
            const int sx = tid / kATY + j * (kAB / kATY);
            const int xx = x0 + sx, yy = y0 + ly;
            if (xx < cols && yy < rows) out[(size_t)xx * (size_t)rows + (size_t)yy] = s_z[sx][ly];
        }
    }
    if (count && tid == 0 && s_count) atomicAdd(count, (unsigned long long)s_count);
}

hipError_t advance_depth_launch(hipStream_t s, const double* field, const double* z, double v2, double w0, double w1, double k, const LinkCamera& cam, int rows,
                                int cols, unsigned long long* plane, double* out, unsigned long long* count) {
    const size_t npix = (size_t)rows * (size_t)cols;
    const dim3 tiles((unsigned)((cols + kATX - 1) / kATX), (unsigned)((rows + kATY - 1) / kATY));
    hipLaunchKernelGGL(advance_preset_kernel, dim3((unsigned)(((npix + 1) / 2 + kAB - 1) / kAB)), dim3(kAB), 0, s, plane, npix);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(advance_splat_kernel, tiles, dim3(kAB), 0, s, field, z, v2, w0, w1, k, cam, rows, cols, plane, count);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(advance_resolve_kernel, tiles, dim3(kAB), 0, s, plane, rows, cols, out, count);
    return hipGetLastError();
}

}  // namespace rsdsfm
