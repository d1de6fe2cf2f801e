// stabilize_blend.hpp -- the stabiliser's seam blend (include/rsdsfm_stabilize_blend.h): what stabilize_blend_kernels.hip and
// stabilize_blend_host.hip share.
#pragma once

#include <stdint.h>

#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_crop.hpp"

namespace rsdsfm {

// tests/stabilize_blend_spec_numpy.py's constants.  The feather and the overlap are choices, not measurements
constexpr int kFeatherDefault = 16, kFeatherMax = 64;
constexpr int64_t kMinOverlapDefault = 1024;
constexpr unsigned kGainMin = 16384u, kGainOne = 65536u, kGainMax = 262144u;

// one channel's gain from the 8-word record [count, sum image_c, sum layer_c, 0 ...]: the spec's gains(); host and device
__host__ __device__ inline unsigned seam_gain(const unsigned long long* sums, int channels, int c, long long min_overlap, int gain_mode) {
    const unsigned long long si = sums[1 + c], sl = sums[1 + channels + c];
    if (gain_mode == 1 || (long long)sums[0] < min_overlap || sl == 0ull) return kGainOne;
    const unsigned long long g = (si * 65536ull + (sl >> 1)) / sl;  // si < 2^36: no overflow
    return g < kGainMin ? kGainMin : g > kGainMax ? kGainMax : (unsigned)g;
}

// DenseWs::d_layer: [distance: P][layer mask: P][layer image: 3 P][one record: 8 uint64], P = rows cols rounded up to 8 bytes; the retimer's
// layer A is this layer (retime_host.hip)
inline size_t blend_plane_bytes(int rows, int cols) { return ((size_t)rows * (size_t)cols + 7u) & ~(size_t)7u; }
inline size_t blend_layer_bytes(int rows, int cols) { return 5 * blend_plane_bytes(rows, cols) + 8 * sizeof(uint64_t); }
struct BlendLayer {
    unsigned char *dist, *mask, *image;
    uint64_t* record;
};
inline BlendLayer blend_layer(unsigned char* d_layer, int rows, int cols) {
    const size_t P = blend_plane_bytes(rows, cols);
    return BlendLayer{d_layer, d_layer + P, d_layer + 2 * P, reinterpret_cast<uint64_t*>(d_layer + 5 * P)};
}

// the two launches of the seam distance on c->stream (arguments checked by the caller): rows, then columns; d_h is the row pass's plane
int seam_distance_launch(Ctx* c, const unsigned char* d_mask, int rows, int cols, int feather, unsigned char* d_h, unsigned char* d_dist);

// the record of one layer on c->stream (arguments checked by the caller): d_sums zeroed by a memset, then the sums launch, which also zeroes
// the blend's two counters when d_counts is passed; the blend launch's front half and rsdsfm_seam_overlap_sums_dev (denoise_host.hip)
int seam_overlap_sums_launch(Ctx* c, const unsigned char* d_image, const unsigned char* d_source, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                             int rows, int cols, unsigned long long* d_sums, unsigned long long* d_counts);

// one layer onto the in-out planes on c->stream (arguments checked by the caller): the record zeroed, the sums launch (which also zeroes
// d_counts), the blend launch
int seam_blend_launch(Ctx* c, const unsigned char* d_layer, const unsigned char* d_lmask, int channels, int rows, int cols, const unsigned char* d_dist, int feather,
                      int64_t min_overlap, int gain_mode, int source_id, unsigned char* d_image, unsigned char* d_mask, unsigned char* d_source,
                      unsigned long long* d_sums, int64_t* d_counts);

}  // namespace rsdsfm
