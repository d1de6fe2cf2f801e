// last_frame.hpp -- the clip's last frame (include/rsdsfm_last_frame.h): what last_frame_kernels.hip and last_frame_host.hip share, and
// what the clip drivers of the stabiliser's stages read of rsdsfm_stabilize_params::last_frame.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/rsdsfm_last_frame.h"
#include "link.hpp"

namespace rsdsfm {

constexpr int kAdvanceLaunches = 3;  // preset, splat, resolve

// One pair's advance on stream s (sides in [2, 16384] and pointers: checked by the caller).  field: rows x cols x 2 row-major; z / out:
// column-major maps; plane: rows x cols uint64 row-major, preset by the first launch; count: NULL or a device counter, zeroed by the splat
// and added to by the resolve (one 64-bit integer atomic per workgroup).
hipError_t advance_depth_launch(hipStream_t s, const double* field, const double* z, double v2, double w0, double w1, double k, const LinkCamera& cam, int rows,
                                int cols, unsigned long long* plane, double* out, unsigned long long* count);

void last_frame_release(Ctx* c);  // last_frame_host.hip: the context's plane (Ctx::last_frame)

// frames a clip call renders: every pair's first frame, and the last frame when the params ask for it (a value the stabiliser's own
// check refuses counts as 0 here: the inner call then returns its error before anything is rendered)
inline int stabilize_rendered_frames(const rsdsfm_stabilize_params* p, int nframes) { return nframes - 1 + ((p && p->last_frame == 1) ? 1 : 0); }

}  // namespace rsdsfm
