// fuse_kernels.hip -- the fusion of a clip's depth maps on MI355X (gfx950): include/rsdsfm_fuse.h, defined by tests/fuse_spec_numpy.py and
// reproduced bit for bit (float64 arithmetic, one rounding per operation, -ffp-contract=off; the numbered steps are the link spec's).  The
// per-pixel expressions are flatten_point's (device_math.hpp), which has no fused form: both library builds compile this file the same way.
//
//   fuse_splat_kernel     link_ratio_kernel's pass up to z_pred: one lane per pixel, splat index in blockIdx.z, a 64 x 16 tile of the
//                         column-major depth map through LDS, the field read row-major (16 B per lane with a depth).  It ends in a 64-bit
//                         unsigned atomicMin of the bit pattern of zf = z_pred * ratio on the landing pixel of the link's plane, which the
//                         host preset to all ones.  A valid depth is a positive finite double, so its pattern orders as an integer: an
//                         exact z-buffer that does not depend on the order of the offers, without a floating atomic.
//   fuse_merge_kernel     one lane per pixel, pair index in blockIdx.z.  Own depth from the LDS tile, the splat word (8 B, row-major), and
//                         -- where the link in front is usable -- the field (16 B) and one gathered double of the next pair's map.  The
//                         fused depth goes back through the LDS tile so that the column-major store coalesces; the flag byte is written
//                         row-major.  The six counters come from ballots: one LDS add per wave, one 64-bit integer atomic per workgroup
//                         and counter.
//
// Algorithmic HBM traffic per pixel and pair: splat 8 B (the plane's preset) + 8 B (Z) + 16 B (field) read and the atomic; merge up to
// 8 B (Z) + 8 B (splat word) + 16 B (field) + 8 B (the gather) read, 8 B + 1 B written.  No private segment.
#include <math.h>

#include "device_math.hpp"
#include "fuse.hpp"

namespace rsdsfm {

namespace {

constexpr int kFB = 256;             // threads of a workgroup: 4 waves
constexpr int kFTX = 64, kFTY = 16;  // tile: 64 columns x 16 rows, 4 pixels per lane
constexpr unsigned long long kNothing = ~0ull;

__device__ __forceinline__ bool valid_depth(double z) { return z > 0.0 && z < INFINITY; }  // finite and > 0; false for NaN
__device__ __forceinline__ bool usable_vector(double2 f) { return fabs(f.x) < INFINITY && fabs(f.y) < INFINITY && !(f.x == 0.0 && f.y == 0.0); }

// the tile of a column-major map into LDS, coalesced along y (as link_ratio_kernel); 0 outside the frame
__device__ __forceinline__ void load_tile(double (*s_z)[kFTY + 1], const double* __restrict__ z, int x0, int y0, int rows, int cols, int tid) {
    const int ly = tid & (kFTY - 1);
#pragma unroll
    for (int j = 0; j < kFTX * kFTY / kFB; ++j) {
        const int lx = tid / kFTY + j * (kFB / kFTY);
        const int xx = x0 + lx, yy = y0 + ly;
        s_z[lx][ly] = (xx < cols && yy < rows) ? z[(size_t)xx * (size_t)rows + (size_t)yy] : 0.0;
    }
}

}  // namespace

// grid: (ceil(cols / kFTX), ceil(rows / kFTY), splats)
__global__ __launch_bounds__(kFB) void fuse_splat_kernel(FuseSplatArgs t, LinkCamera cam, int rows, int cols) {
    __shared__ double s_z[kFTX][kFTY + 1];
    const int l = blockIdx.z;
    const double ratio = t.ratio[l];
    if (!(ratio > 0.0)) return;  // (the whole workgroup) a link that is not usable: its plane keeps the preset
    const double* __restrict__ field = t.field[l];
    unsigned long long* __restrict__ plane = t.plane[l];
    const double v2 = t.v2[l], w0 = t.w0[l], w1 = t.w1[l], k = t.k[l];
    const int x0 = (int)blockIdx.x * kFTX, y0 = (int)blockIdx.y * kFTY;
    const int tid = (int)threadIdx.x;
    load_tile(s_z, t.z[l], x0, y0, rows, cols, tid);
    __syncthreads();
    const int lx = tid & (kFTX - 1), x = x0 + lx;
    const int wv = tid / kFTX;
    const double h = (double)rows;
#pragma unroll
    for (int j = 0; j < kFTY / (kFB / kFTX); ++j) {
        const int ly = wv + j * (kFB / kFTX);
        const int y = y0 + ly;  // wave-uniform
        if (!(x < cols && y < rows)) continue;
        const double z = s_z[lx][ly];
        if (!valid_depth(z)) continue;
        const size_t idx = (size_t)y * (size_t)cols + (size_t)x;
        const double2 f = make_double2(field[2 * idx], field[2 * idx + 1]);
        if (!usable_vector(f)) continue;
        const FlatPoint p = flatten_point(f, x, y, cam.fx, cam.fy, cam.cx, cam.cy, cam.gamma, h);                    // 1
        const double alpha = cam.global_shutter ? 1.0 : p.alpha;
        const double beta = (2.0 * (alpha + k * p.alpha_k)) / (2.0 + k);                                               // 2
        const double b = beta / cam.gamma;
        const double z_pred = z * (1.0 + b * (w0 * p.qy - w1 * p.qx)) + b * v2;                                        // 3
        const double r2 = floor(((double)y + f.y) + 0.5), c2 = floor(((double)x + f.x) + 0.5);                         // 4
        const bool inside = r2 >= 0.0 && r2 <= (double)(rows - 1) && c2 >= 0.0 && c2 <= (double)(cols - 1);
        const double zf = z_pred * ratio;
        if (inside && valid_depth(zf))
            atomicMin(&plane[(size_t)(int)r2 * (size_t)cols + (size_t)(int)c2], (unsigned long long)__double_as_longlong(zf));  // inside the plane
    }
}

// grid: (ceil(cols / kFTX), ceil(rows / kFTY), pairs)
__global__ __launch_bounds__(kFB) void fuse_merge_kernel(FuseMergeArgs t, LinkCamera cam, int rows, int cols, double tol,
                                                         unsigned long long* __restrict__ counters) {
    __shared__ double s_z[kFTX][kFTY + 1];
    __shared__ int s_count[kFuseCounters];
    const int l = blockIdx.z;
    const double* __restrict__ field = t.field[l];
    const double* __restrict__ zn = t.zn[l];
    const unsigned long long* __restrict__ plane = t.plane[l];
    uint8_t* __restrict__ flags = t.flags[l];
    const double v2 = t.v2[l], w0 = t.w0[l], w1 = t.w1[l], k = t.k[l], ratio = t.ratio[l];
    const bool has_next = ratio > 0.0;
    const int x0 = (int)blockIdx.x * kFTX, y0 = (int)blockIdx.y * kFTY;
    const int tid = (int)threadIdx.x;
    if (tid < kFuseCounters) s_count[tid] = 0;
    load_tile(s_z, t.z[l], x0, y0, rows, cols, tid);
    __syncthreads();
    const int lx = tid & (kFTX - 1), x = x0 + lx;
    const int wv = tid / kFTX;
    const double h = (double)rows;
    const double onetol = 1.0 + tol;
    int n_own = 0, n_prev = 0, n_next = 0, n_conf = 0, n_contra = 0, n_left = 0;
#pragma unroll
    for (int j = 0; j < kFTY / (kFB / kFTX); ++j) {
        const int ly = wv + j * (kFB / kFTX);
        const int y = y0 + ly;  // wave-uniform
        const bool live = x < cols && y < rows;
        bool own = false, prev = false, nxt = false, pa = false, na = false;
        if (live) {
            const double z = s_z[lx][ly];
            const size_t idx = (size_t)y * (size_t)cols + (size_t)x;
            own = valid_depth(z);
            double zprev = 0.0, zc = 0.0;
            if (plane) {
                const unsigned long long word = plane[idx];
                prev = word != kNothing;
                zprev = __longlong_as_double((long long)word);
            }
            if (has_next) {
                const double2 f = make_double2(field[2 * idx], field[2 * idx + 1]);
                const double r2 = floor(((double)y + f.y) + 0.5), c2 = floor(((double)x + f.x) + 0.5);                 // 4
                const bool inside = r2 >= 0.0 && r2 <= (double)(rows - 1) && c2 >= 0.0 && c2 <= (double)(cols - 1);
                if (usable_vector(f) && inside) {
                    const double z2 = zn[(size_t)(int)c2 * (size_t)rows + (size_t)(int)r2];  // inside the map
                    if (valid_depth(z2)) {
                        const FlatPoint p = flatten_point(f, x, y, cam.fx, cam.fy, cam.cx, cam.cy, cam.gamma, h);    // 1
                        const double alpha = cam.global_shutter ? 1.0 : p.alpha;
                        const double beta = (2.0 * (alpha + k * p.alpha_k)) / (2.0 + k);                               // 2
                        const double b = beta / cam.gamma;
                        zc = (z2 / ratio - b * v2) / (1.0 + b * (w0 * p.qy - w1 * p.qx));                              // 3, solved for z
                        nxt = valid_depth(zc);
                    }
                }
            }
            const double fz = own ? z : (prev ? zprev : (nxt ? zc : 0.0));
            pa = prev && zprev <= fz * onetol && zprev * onetol >= fz;
            na = nxt && zc <= fz * onetol && zc * onetol >= fz;
            s_z[lx][ly] = fz;  // (the lane's own cell)
            if (flags) flags[idx] = (uint8_t)((own ? 1 : 0) | (prev ? 2 : 0) | (nxt ? 4 : 0) | (pa ? 8 : 0) | (na ? 16 : 0));
        }
        n_own += (int)__popcll(__ballot(own));
        n_prev += (int)__popcll(__ballot(live && !own && prev));
        n_next += (int)__popcll(__ballot(live && !own && !prev && nxt));
        n_conf += (int)__popcll(__ballot(own && (pa || na)));
        n_contra += (int)__popcll(__ballot(own && ((prev && !pa) || (nxt && !na))));
        n_left += (int)__popcll(__ballot(live && !own && !prev && !nxt));
    }
    if ((tid & 63) == 0) {
        if (n_own) atomicAdd(&s_count[0], n_own);
        if (n_prev) atomicAdd(&s_count[1], n_prev);
        if (n_next) atomicAdd(&s_count[2], n_next);
        if (n_conf) atomicAdd(&s_count[3], n_conf);
        if (n_contra) atomicAdd(&s_count[4], n_contra);
        if (n_left) atomicAdd(&s_count[5], n_left);
    }
    __syncthreads();  // the tile holds the fused depths, the counts are complete
    {
        double* __restrict__ fused = t.fused[l];
        const int ly = tid & (kFTY - 1);
#pragma unroll
        for (int j = 0; j < kFTX * kFTY / kFB; ++j) {
            const int sx = tid / kFTY + j * (kFB / kFTY);
            const int xx = x0 + sx, yy = y0 + ly;
            if (xx < cols && yy < rows) fused[(size_t)xx * (size_t)rows + (size_t)yy] = s_z[sx][ly];
        }
    }
    if (tid < kFuseCounters && s_count[tid]) atomicAdd(&counters[(size_t)l * kFuseCounters + tid], (unsigned long long)s_count[tid]);
}

hipError_t fuse_splat_launch(hipStream_t s, const FuseSplatArgs& a, const LinkCamera& cam, int n, int rows, int cols) {
    const dim3 tiles((unsigned)((cols + kFTX - 1) / kFTX), (unsigned)((rows + kFTY - 1) / kFTY), (unsigned)n);
    hipLaunchKernelGGL(fuse_splat_kernel, tiles, dim3(kFB), 0, s, a, cam, rows, cols);
    return hipGetLastError();
}

hipError_t fuse_merge_launch(hipStream_t s, const FuseMergeArgs& a, const LinkCamera& cam, int n, int rows, int cols, double tol,
                             unsigned long long* counters) {
    const dim3 tiles((unsigned)((cols + kFTX - 1) / kFTX), (unsigned)((rows + kFTY - 1) / kFTY), (unsigned)n);
    hipLaunchKernelGGL(fuse_merge_kernel, tiles, dim3(kFB), 0, s, a, cam, rows, cols, tol, counters);
    return hipGetLastError();
}

}  // namespace rsdsfm
