// link.hpp -- the link between consecutive pairs of a clip and the clip's points (include/rsdsfm_trajectory.h): what link_kernels.hip and
// link_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "flow_kernels.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

constexpr int kLinkMax = kFlowSeqMaxPairs;  // links of one set of launches (link index = blockIdx.z)
constexpr int kLinkMaxBits = 11;            // widest radix digit: 2048 bins, 8 KB of LDS per workgroup
constexpr int kLinkBins = 1 << kLinkMaxBits;
constexpr int kPointsMax = 16;              // pairs of one clip-points launch (their transforms travel in the kernel arguments)

// The links of one set of launches, kernel-argument tables as flow_enqueue's.  Link l reads the field and the depth map of pair p (column-major)
// and the depth map of pair p + 1, and writes its ratio plane (rows x cols uint64, row-major: the caller's buffer or the workspace's).
struct LinkPtrs {
    const double* field[kLinkMax];
    const double* zp[kLinkMax];
    const double* zn[kLinkMax];
    unsigned long long* plane[kLinkMax];
};
// what the link reads of pair p's motion: v[2], w[0], w[1] and k
struct LinkMotion {
    double v2[kLinkMax], w0[kLinkMax], w1[kLinkMax], k[kLinkMax];
};
struct LinkCamera {
    double fx, fy, cx, cy, gamma;
    int global_shutter;
};
// per-link device state (zero when the ratio pass starts): the counters, and the selection's prefix (the digits picked so far; the median's
// bit pattern after the last pass) and the rank that remains among the patterns with that prefix
struct LinkState {
    unsigned long long n, agree, prefix, rank;
};
struct PointsArgs {
    const float* in[kPointsMax];
    float* out[kPointsMax];
    double scale[kPointsMax];
    double A[kPointsMax][9];
    double c[kPointsMax][3];
};

// nlinks <= kLinkMax links of rows x cols pixels (sides in [2, 16384]: checked by the caller).  hist: nlinks x kLinkBins zeroed words;
// state: nlinks zeroed LinkState.  bits = 8 or 11.  The launches: the ratio pass, ceil(64 / bits) x (histogram, pick), the agree pass.
hipError_t link_launch(hipStream_t s, const LinkPtrs& t, const LinkMotion& m, const LinkCamera& cam, int nlinks, int rows, int cols, int bits, double tol,
                       unsigned* hist, LinkState* state);
int link_launch_count(int bits);

// npairs <= kPointsMax pairs in one launch
hipError_t clip_points_launch(hipStream_t s, const PointsArgs& a, int npairs, int64_t npix);

void link_rodrigues(const double a[3], double R[9]);  // link_host.hip: the chain's exp([a]x), row-major (host); the stabiliser's too
void link_release(Ctx* c);  // link_host.hip: the context's link workspace (Ctx::link)

}  // namespace rsdsfm
