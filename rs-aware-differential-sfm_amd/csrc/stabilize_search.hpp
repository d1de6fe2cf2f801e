// stabilize_search.hpp -- the stabiliser's search for the visible pre-image (include/rsdsfm_stabilize_search.h): what
// stabilize_search_kernels.hip, stabilize_search_host.hip and the clip loops that render neighbours (stabilize_fill_host.hip,
// stabilize_crop_host.hip, stabilize_blend_host.hip) share.
#pragma once

#include <stdint.h>

#include "../../include/rsdsfm_stabilize_search.h"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize.hpp"
#include "stabilize_visible.hpp"

namespace rsdsfm {

constexpr unsigned long long kKeyEmpty = ~0ull;  // no source pixel landed on the cell
constexpr unsigned kKeyHighEmpty = ~0u;

// the two planes of the search (DenseWs::d_search: [kbuf: rows x cols uint64][zv: rows x cols float]); the keys first, for their alignment
struct SearchWs {
    unsigned long long* d_kbuf;
    float* d_zv;
};
inline SearchWs search_ws_layout(void* d_search, int rows, int cols) {
    unsigned long long* kbuf = static_cast<unsigned long long*>(d_search);
    return SearchWs{kbuf, reinterpret_cast<float*>(kbuf + (size_t)rows * (size_t)cols)};
}
inline size_t search_ws_bytes(int rows, int cols) { return 12 * (size_t)rows * (size_t)cols; }

// rsdsfm_set_occlusion_search: a clip call's neighbour candidates that go through the occlusion test go through the search call
inline bool search_asked(const Ctx* c, const rsdsfm_stabilize_fill_params* fp) { return visible_asked(fp) && c->occlusion_search == 1; }
// int64 counters per candidate of a clip loop: the plain calls' count, [taken, rejected], [taken, rejected, recovered]
inline int candidate_counters(bool occ, bool search) { return search ? 3 : occ ? 2 : 1; }
// what a candidate put into the frame: a recovered pixel counts under its offset
inline int64_t candidate_count(const int64_t* cnt, bool search) { return search ? cnt[0] + cnt[2] : cnt[0]; }

// the launches of one frame through a window, the test and the search on c->stream (arguments checked by the caller; iterations 1 .. 16;
// tol_q16 1 .. 65536): the dense rectifier's stage A, the byte memset of kbuf, the map kernel that also writes zv and splats the keys, and
// the warp kernel that tests, searches and counts; as stabilize_visible_launch otherwise
int stabilize_search_launch(Ctx* c, const DenseWs& ws, const SearchWs& sw, const unsigned char* d_img_n, int channels, const double* d_depth_cm, const double* d_R,
                            const double* d_t, double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp,
                            int source_id, const int32_t window[4], unsigned char* d_out, unsigned char* d_mask, unsigned char* d_source, int tol_q16,
                            int64_t* d_counts3);

}  // namespace rsdsfm
