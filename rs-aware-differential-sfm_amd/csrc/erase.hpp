// erase.hpp -- the mover removal (include/rsdsfm_erase.h): what erase_kernels.hip and erase_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_erase.h"
#include "plate.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {

// tests/erase_spec_numpy.py's constants.  The defaults are choices, not measurements
constexpr int kEraseOpenMax = RSDSFM_ERASE_OPEN_MAX, kEraseOpenDefault = RSDSFM_ERASE_OPEN_DEFAULT;
constexpr int kEraseGrowMax = RSDSFM_ERASE_GROW_MAX, kEraseGrowDefault = RSDSFM_ERASE_GROW_DEFAULT;
constexpr int kEraseFeatherMax = RSDSFM_ERASE_FEATHER_MAX, kEraseFeatherDefault = RSDSFM_ERASE_FEATHER_DEFAULT;
constexpr int kEraseReachMax = kEraseOpenMax + kEraseGrowMax + kEraseFeatherMax;  // C <= 27
constexpr int kEraseHaloMax = kEraseOpenMax + kEraseReachMax - 1;                 // the row pass's halo, o + C - 1 <= 29

// DenseWs::d_matte: [the seeds ANDed over the rows: P][the row distance: P]
// DenseWs::d_erase: [plate mask: P][flag: P][matte: P][plate image: 3 P], P = blend_plane_bytes (a multiple of 8: every plane 4-byte aligned)
inline size_t matte_ws_bytes(int rows, int cols) { return 2 * blend_plane_bytes(rows, cols); }
inline size_t erase_ws_bytes(int rows, int cols) { return 6 * blend_plane_bytes(rows, cols); }

// the matte's three launches on c->stream (arguments checked by the caller; literal o, g, T): d_v and d_h are the two intermediate planes
int mover_matte_launch(Ctx* c, const unsigned char* d_flag, int rows, int cols, int open, int grow, int feather, int include_undecided, unsigned char* d_v,
                       unsigned char* d_h, unsigned char* d_matte);

// the composite on c->stream (arguments checked by the caller): the counters zeroed by a memset when passed, then one launch
int erase_composite_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_plate, const unsigned char* d_pmask,
                           const unsigned char* d_matte, int channels, int rows, int cols, int feather, unsigned char* d_out, unsigned char* d_mask_out, int64_t* d_counts5);

}  // namespace rsdsfm
