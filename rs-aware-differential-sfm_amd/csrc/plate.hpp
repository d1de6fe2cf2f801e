// plate.hpp -- the clean plate (include/rsdsfm_plate.h): what plate_kernels.hip and plate_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_plate_medoid.h"
#include "denoise.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {

constexpr int kPlateRadiusMax = RSDSFM_PLATE_RADIUS_MAX;
constexpr int kPlateLayersMax = RSDSFM_PLATE_LAYERS_MAX;
constexpr int kPlateSourcesMax = 1 + kPlateLayersMax;  // 15 candidates at most: the own frame and 14 neighbours
constexpr int kPlateThresholdDefault = RSDSFM_PLATE_THRESHOLD_DEFAULT, kPlateThresholdMax = 255;
constexpr int kPlateMinVotesDefault = RSDSFM_PLATE_MIN_VOTES_DEFAULT, kPlateMinVotesMax = kPlateSourcesMax;
static_assert(kPlateLayersMax == kDenoiseLayersMax, "the plate walks a clip as the denoise does");

// the layer counts the kernel is compiled for: a call with L layers runs the smallest of them that holds L, the layers beyond L never read
constexpr int kPlateSizes[] = {0, 2, 4, 7, 14};
constexpr int kPlateNumSizes = 5;

// the kernel's argument: the planes travel in the kernel argument itself (15 + 15 pointers, 1 record pointer), no pointer table in global memory
struct PlateArgs {
    const unsigned char* ref;
    const unsigned char* rmask;
    const unsigned char* layer[kPlateLayersMax];
    const unsigned char* lmask[kPlateLayersMax];
    const unsigned long long* sums;  // nlayers x 8, or NULL
    unsigned char* out;
    unsigned char* mask_out;
    unsigned char* votes;   // or NULL
    unsigned char* moving;  // or NULL
    unsigned long long* counts;  // [unset, static, moving, undecided], or NULL
    long long min_overlap;
    int rows, cols, nlayers, gain_mode;
    unsigned threshold, min_votes;
};

// DenseWs::d_plate: [reference mask: P][reference source: P][reference image: 3 P][records: 14 x 8 uint64][layer 0 mask: P][layer 0 image: 3 P]
// [layer 1 ...], P = blend_plane_bytes (a multiple of 8, so the records are 8-byte aligned and every plane 4)
inline size_t plate_records_bytes() { return (size_t)kPlateLayersMax * 8 * sizeof(uint64_t); }
inline size_t plate_ws_bytes(int rows, int cols, int layers) { return (5 + 4 * (size_t)layers) * blend_plane_bytes(rows, cols) + plate_records_bytes(); }
struct PlatePlanes {
    unsigned char *rmask, *rsource, *rimage;
    uint64_t* records;
    unsigned char* stack;  // layer j: its mask at stack + 4 P j, its image P behind
};
inline PlatePlanes plate_planes(unsigned char* d_plate, int rows, int cols) {
    const size_t P = blend_plane_bytes(rows, cols);
    return PlatePlanes{d_plate, d_plate + P, d_plate + 2 * P, reinterpret_cast<uint64_t*>(d_plate + 5 * P), d_plate + 5 * P + plate_records_bytes()};
}

// the params with every 0 of radius, threshold, min_votes and min_overlap replaced by its default, or the defaults for NULL; false: refused with
// kPlateParamsMessage (plate_host.hip; the mover removal resolves the plate's fields of its own params with it)
bool plate_params_resolve(const rsdsfm_plate_params* in, rsdsfm_plate_params* out);
extern const char* const kPlateParamsMessage;

// the median on c->stream (arguments checked by the caller): the counters zeroed by a memset when passed, then one launch
int plate_median_launch(Ctx* c, const PlateArgs& args, int channels);
// the L1 medoid in its place (include/rsdsfm_plate_medoid.h; plate_medoid_kernels.hip): the same memset, one launch; channels == 1 IS the median's
int plate_medoid_launch(Ctx* c, const PlateArgs& args, int channels);

}  // namespace rsdsfm
