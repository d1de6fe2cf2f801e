// fuse.hpp -- the fusion of a clip's depth maps (include/rsdsfm_fuse.h): what fuse_kernels.hip and fuse_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "link.hpp"

namespace rsdsfm {

constexpr int kFuseCounters = 6;  // own, filled_prev, filled_next, confirmed, contradicted, left: rsdsfm_fuse_record's order

// The splats of one launch, kernel-argument tables as LinkPtrs.  Splat l reads the field and the depth map (column-major) of the pair in
// front of the link and lowers its plane (rows x cols uint64, row-major, preset to all ones) with 64-bit integer atomics.  ratio = 0
// marks a link that is not usable: its workgroups return at once and the plane keeps its preset.
struct FuseSplatArgs {
    const double* field[kLinkMax];
    const double* z[kLinkMax];
    unsigned long long* plane[kLinkMax];
    double v2[kLinkMax], w0[kLinkMax], w1[kLinkMax], k[kLinkMax], ratio[kLinkMax];
};
// The merges of one launch.  Pair l reads its own map z, the plane of the link behind it (NULL: no previous pair, or a link that is not
// usable) and, when ratio > 0, its field and the next pair's map zn; writes fused (column-major), flags (row-major; may be NULL) and adds
// to its kFuseCounters counters.
struct FuseMergeArgs {
    const double* field[kLinkMax];
    const double* z[kLinkMax];
    const double* zn[kLinkMax];
    const unsigned long long* plane[kLinkMax];
    double* fused[kLinkMax];
    uint8_t* flags[kLinkMax];
    double v2[kLinkMax], w0[kLinkMax], w1[kLinkMax], k[kLinkMax], ratio[kLinkMax];
};

// n <= kLinkMax splats / merges of rows x cols pixels (sides in [2, 16384]: checked by the caller), one launch each
hipError_t fuse_splat_launch(hipStream_t s, const FuseSplatArgs& a, const LinkCamera& cam, int n, int rows, int cols);
// counters: n x kFuseCounters zeroed words
hipError_t fuse_merge_launch(hipStream_t s, const FuseMergeArgs& a, const LinkCamera& cam, int n, int rows, int cols, double tol,
                             unsigned long long* counters);

void fuse_release(Ctx* c);  // fuse_host.hip: the context's fusion workspace (Ctx::fuse)

}  // namespace rsdsfm
