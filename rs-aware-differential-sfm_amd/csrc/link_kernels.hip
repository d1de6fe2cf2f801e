// link_kernels.hip -- the link between consecutive pairs of a clip on MI355X (gfx950): include/rsdsfm_trajectory.h, defined by
// tests/link_spec_numpy.py and reproduced bit for bit (float64 arithmetic, one rounding per operation, -ffp-contract=off; the numbered
// steps below are the spec's).  The per-pixel expressions are flatten_point's (device_math.hpp), which has no fused form: both library
// builds compile this file the same way.
//
//   link_ratio_kernel     one lane per pixel, link index in blockIdx.z.  A 64 x 16 tile of pair p's column-major depth map goes through LDS
//                         (coalesced along y, as depth_claim and rectify_dense_pull0), the field is read row-major (16 B per lane), one double
//                         of pair p + 1's map is gathered at the landing pixel (a few pixels away: L2), and the ratio's bit pattern, or 0
//                         for "no correspondence", is written to the link's plane (8 B).  n is counted from the ballots, per workgroup in
//                         LDS, with one 64-bit integer atomic per workgroup.
//   link_hist_kernel      one radix pass of the exact selection: a valid ratio is a positive finite double, so its bit pattern orders as a
//                         uint64.  Every pattern that carries the prefix picked so far adds one to its digit's bin: integer atomics in an LDS
//                         histogram, whose non-empty bins go to the link's histogram in HBM with one integer atomic each.
//   link_pick_kernel      one workgroup per link: finds the bin that holds the remaining rank, appends the digit to the prefix, takes the
//                         bins below it off the rank, and zeroes the histogram for the next pass.  After the last pass the prefix IS the
//                         lower median's bit pattern.  No host wait between passes, no floating sum: exact and independent of scheduling.
//   link_agree_kernel     one more streaming pass over the plane: the patterns within tol of the median, counted like n.
//   clip_points_kernel    A (S X) + c per point, float64, rounded once to float; (0, 0, 0) stays (0, 0, 0).  One lane per point, the pair in
//                         blockIdx.z, the transforms in the kernel arguments.
//
// Algorithmic HBM traffic per pixel and link: 8 B (Z_p) + 16 B (field) + up to 8 B (the gather of Z_{p+1}) read and 8 B written by the
// ratio pass, 8 B read by each of the ceil(64 / bits) radix passes and by the agree pass.  No private segment.
#include <math.h>

#include "device_math.hpp"
#include "link.hpp"

namespace rsdsfm {

namespace {

constexpr int kLB = 256;            // threads of a workgroup: 4 waves
constexpr int kLTX = 64, kLTY = 16;  // tile of the ratio pass: 64 columns x 16 rows, 4 pixels per lane
constexpr int kPer = 8;             // patterns per lane of the streaming passes

__device__ __forceinline__ bool valid_depth(double z) { return z > 0.0 && z < INFINITY; }  // finite and > 0; false for NaN

}  // namespace

// grid: (ceil(cols / kLTX), ceil(rows / kLTY), links)
__global__ __launch_bounds__(kLB) void link_ratio_kernel(LinkPtrs t, LinkMotion m, LinkCamera cam, int rows, int cols, LinkState* __restrict__ state) {
    __shared__ double s_z[kLTX][kLTY + 1];
    __shared__ int s_count;
    const int link = blockIdx.z;
    const double* __restrict__ field = t.field[link];
    const double* __restrict__ zp = t.zp[link];
    const double* __restrict__ zn = t.zn[link];
    unsigned long long* __restrict__ plane = t.plane[link];
    const double v2 = m.v2[link], w0 = m.w0[link], w1 = m.w1[link], k = m.k[link];
    const int x0 = (int)blockIdx.x * kLTX, y0 = (int)blockIdx.y * kLTY;
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_count = 0;
    {
        const int ly = tid & (kLTY - 1);
#pragma unroll
        for (int j = 0; j < kLTX * kLTY / kLB; ++j) {
            const int lx = tid / kLTY + j * (kLB / kLTY);
            const int xx = x0 + lx, yy = y0 + ly;
            s_z[lx][ly] = (xx < cols && yy < rows) ? zp[(size_t)xx * (size_t)rows + (size_t)yy] : 0.0;
        }
    }
    __syncthreads();
    const int lx = tid & (kLTX - 1), x = x0 + lx;
    const int wv = tid / kLTX;
    const double h = (double)rows;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < kLTY / (kLB / kLTX); ++j) {
        const int ly = wv + j * (kLB / kLTX);
        const int y = y0 + ly;  // wave-uniform
        const bool live = x < cols && y < rows;
        bool ok = false;
        double ratio = 0.0;
        if (live) {
            const double z = s_z[lx][ly];
            const size_t idx = (size_t)y * (size_t)cols + (size_t)x;
            const double2 f = make_double2(field[2 * idx], field[2 * idx + 1]);
            if (valid_depth(z)) {
                const FlatPoint p = flatten_point(f, x, y, cam.fx, cam.fy, cam.cx, cam.cy, cam.gamma, h);                    // 1
                const double alpha = cam.global_shutter ? 1.0 : p.alpha;
                const double beta = (2.0 * (alpha + k * p.alpha_k)) / (2.0 + k);                                               // 2
                const double b = beta / cam.gamma;
                const double z_pred = z * (1.0 + b * (w0 * p.qy - w1 * p.qx)) + b * v2;                                        // 3
                const double r2 = floor(((double)y + f.y) + 0.5), c2 = floor(((double)x + f.x) + 0.5);                         // 4
                const bool inside = r2 >= 0.0 && r2 <= (double)(rows - 1) && c2 >= 0.0 && c2 <= (double)(cols - 1);
                if (inside && valid_depth(z_pred)) {
                    const double z2 = zn[(size_t)(int)c2 * (size_t)rows + (size_t)(int)r2];  // inside the map                    5
                    if (valid_depth(z2)) {
                        ratio = z2 / z_pred;
                        ok = valid_depth(ratio);                                                                               // 6
                    }
                }
            }
            plane[idx] = ok ? (unsigned long long)__double_as_longlong(ratio) : 0ull;                                         // 7
        }
        mine += (int)__popcll(__ballot(ok));
    }
    if ((tid & 63) == 0 && mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (tid == 0 && s_count) atomicAdd(&state[link].n, (unsigned long long)s_count);
}

// grid: (ceil(npix / (kLB * kPer)), 1, links); shift = the digit's lowest bit, bits = its width
__global__ __launch_bounds__(kLB) void link_hist_kernel(LinkPtrs t, int64_t npix, int shift, int bits, const LinkState* __restrict__ state,
                                                        unsigned* __restrict__ hist) {
    __shared__ unsigned s_hist[kLinkBins];
    const int link = blockIdx.z;
    const unsigned long long* __restrict__ plane = t.plane[link];
    const int nb = 1 << bits;
    const int tid = (int)threadIdx.x;
    for (int b = tid; b < nb; b += kLB) s_hist[b] = 0u;
    __syncthreads();
    const bool whole = shift + bits >= 64;  // the first pass: every pattern takes part
    const unsigned long long prefix = state[link].prefix;
    const int64_t base = (int64_t)blockIdx.x * (kLB * kPer) + tid;
    unsigned long long v[kPer];
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        const int64_t i = base + (int64_t)e * kLB;
        v[e] = i < npix ? plane[i] : 0ull;
    }
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        const bool take = v[e] != 0ull && (whole || (v[e] >> (shift + bits)) == prefix);
        if (take) atomicAdd(&s_hist[(unsigned)(v[e] >> shift) & (unsigned)(nb - 1)], 1u);
    }
    __syncthreads();
    unsigned* __restrict__ out = hist + (size_t)link * kLinkBins;
    for (int b = tid; b < nb; b += kLB) {
        const unsigned cnt = s_hist[b];
        if (cnt) atomicAdd(&out[b], cnt);
    }
}

// grid: (links); one workgroup per link.  first: the rank is set from n here ((n - 1) / 2, the lower median)
__global__ __launch_bounds__(kLB) void link_pick_kernel(int bits, int first, LinkState* __restrict__ state, unsigned* __restrict__ hist) {
    constexpr int kOwn = kLinkBins / kLB;  // bins per lane at the widest digit
    __shared__ unsigned long long s_sum[kLB];
    __shared__ int s_owner;
    __shared__ unsigned long long s_below;
    const int link = blockIdx.x;
    const int tid = (int)threadIdx.x;
    const int nb = 1 << bits;
    unsigned* __restrict__ h = hist + (size_t)link * kLinkBins;
    const unsigned long long n = state[link].n;
    const unsigned long long rank = first ? (n ? (n - 1ull) / 2ull : 0ull) : state[link].rank;
    const unsigned long long prefix = first ? 0ull : state[link].prefix;
    unsigned own[kOwn];
    unsigned long long sum = 0ull;
#pragma unroll
    for (int e = 0; e < kOwn; ++e) {
        const int b = tid * kOwn + e;
        own[e] = b < nb ? h[b] : 0u;
        sum += own[e];
    }
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        // the lane whose bins hold the rank: the first one at which the running count exceeds it (none when the link has no correspondence)
        unsigned long long below = 0ull;
        int owner = -1;
        for (int l = 0; l < kLB; ++l) {
            if (below + s_sum[l] > rank) {
                owner = l;
                break;
            }
            below += s_sum[l];
        }
        s_owner = owner, s_below = below;
    }
    __syncthreads();
    const int owner = s_owner;
    if (owner < 0) {
        if (tid == 0) state[link].prefix = prefix << bits, state[link].rank = 0ull;
    } else if (tid == owner) {
        unsigned long long below = s_below;
        unsigned digit = 0u;
#pragma unroll
        for (int e = 0; e < kOwn; ++e) {
            if (below + own[e] > rank) {
                digit = (unsigned)(tid * kOwn + e);
                break;
            }
            below += own[e];
        }
        state[link].prefix = (prefix << bits) | (unsigned long long)digit;
        state[link].rank = rank - below;
    }
#pragma unroll
    for (int e = 0; e < kOwn; ++e) {
        const int b = tid * kOwn + e;
        if (b < nb && own[e]) h[b] = 0u;
    }
}

// grid: (ceil(npix / (kLB * kPer)), 1, links)
__global__ __launch_bounds__(kLB) void link_agree_kernel(LinkPtrs t, int64_t npix, double tol, LinkState* __restrict__ state) {
    __shared__ int s_count;
    const int link = blockIdx.z;
    const unsigned long long* __restrict__ plane = t.plane[link];
    const int tid = (int)threadIdx.x;
    if (tid == 0) s_count = 0;
    __syncthreads();
    const double med = __longlong_as_double((long long)state[link].prefix);
    const double onetol = 1.0 + tol;
    const double hi = med * onetol;
    const int64_t base = (int64_t)blockIdx.x * (kLB * kPer) + tid;
    int mine = 0;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        const int64_t i = base + (int64_t)e * kLB;
        const unsigned long long v = i < npix ? plane[i] : 0ull;
        const double r = __longlong_as_double((long long)v);
        const bool ok = v != 0ull && r <= hi && r * onetol >= med;
        mine += (int)__popcll(__ballot(ok));
    }
    if ((tid & 63) == 0 && mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (tid == 0 && s_count) atomicAdd(&state[link].agree, (unsigned long long)s_count);
}

// grid: (ceil(npix / kLB), 1, pairs)
__global__ __launch_bounds__(kLB) void clip_points_kernel(PointsArgs a, int64_t npix) {
    const int pair = blockIdx.z;
    const int64_t i = (int64_t)blockIdx.x * kLB + (int)threadIdx.x;
    if (i >= npix) return;
    const float* in = a.in[pair];  // (out may be in: a lane reads its own point before it writes it)
    float* out = a.out[pair];
    const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
    if (!(x == 0.0f && y == 0.0f && z == 0.0f)) {
        const double s = a.scale[pair];
        const double p0 = s * (double)x, p1 = s * (double)y, p2 = s * (double)z;
        const double* A = a.A[pair];
        const double* c = a.c[pair];
        o0 = (float)(((A[0] * p0 + A[1] * p1) + A[2] * p2) + c[0]);
        o1 = (float)(((A[3] * p0 + A[4] * p1) + A[5] * p2) + c[1]);
        o2 = (float)(((A[6] * p0 + A[7] * p1) + A[8] * p2) + c[2]);
    }
    out[3 * i] = o0, out[3 * i + 1] = o1, out[3 * i + 2] = o2;
}

int link_launch_count(int bits) { return 2 + 2 * ((64 + bits - 1) / bits); }

hipError_t link_launch(hipStream_t s, const LinkPtrs& t, const LinkMotion& m, const LinkCamera& cam, int nlinks, int rows, int cols, int bits, double tol,
                       unsigned* hist, LinkState* state) {
    const int64_t npix = (int64_t)rows * cols;  // <= 2^28
    const dim3 tiles((unsigned)((cols + kLTX - 1) / kLTX), (unsigned)((rows + kLTY - 1) / kLTY), (unsigned)nlinks);
    const dim3 stream_grid((unsigned)((npix + kLB * kPer - 1) / (kLB * kPer)), 1u, (unsigned)nlinks);
    hipLaunchKernelGGL(link_ratio_kernel, tiles, dim3(kLB), 0, s, t, m, cam, rows, cols, state);
    const int passes = (64 + bits - 1) / bits;
    for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(link_hist_kernel, stream_grid, dim3(kLB), 0, s, t, npix, bits * (passes - 1 - p), bits, state, hist);
        hipLaunchKernelGGL(link_pick_kernel, dim3((unsigned)nlinks), dim3(kLB), 0, s, bits, p == 0 ? 1 : 0, state, hist);
    }
    hipLaunchKernelGGL(link_agree_kernel, stream_grid, dim3(kLB), 0, s, t, npix, tol, state);
    return hipGetLastError();
}

hipError_t clip_points_launch(hipStream_t s, const PointsArgs& a, int npairs, int64_t npix) {
    hipLaunchKernelGGL(clip_points_kernel, dim3((unsigned)((npix + kLB - 1) / kLB), 1u, (unsigned)npairs), dim3(kLB), 0, s, a, npix);
    return hipGetLastError();
}

}  // namespace rsdsfm
