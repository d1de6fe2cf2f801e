// clip_stage_host.hpp -- what the hosts of the image stages behind the stabiliser share (retime, shutter, denoise, super-resolution, clean
// plate, and the fill, crop, blend and inpaint clip calls): the small argument checks, one frame's sources and poses (ClipPlan), the three-way
// choice of the render entry point for a neighbour candidate, the device counters of a clip call, and the clip walk of the stages that render
// every frame from its registered neighbours.  Helpers that report take the stage's message prefix.  DESIGN section 12, "Shared tile toolkit
// and clip walk".
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "rsdsfm_internal.hpp"

namespace rsdsfm {

inline bool finite_all(const double* a, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

inline bool frame_size_ok(int rows, int cols, int max = 16384) { return rows >= 2 && cols >= 2 && rows <= max && cols <= max; }

// (r0, c0, h, w): given, h >= 1, w >= 1 and inside the frame
inline bool window_ok(const int32_t* w, int rows, int cols) {
    return w && w[2] >= 1 && w[3] >= 1 && w[0] >= 0 && w[1] >= 0 && (int64_t)w[0] + w[2] <= rows && (int64_t)w[1] + w[3] <= cols;
}

// the caller's window, or the whole frame written to `full`; NULL: the caller's window is refused
inline const int32_t* window_or_full(const int32_t* window_or_null, int rows, int cols, int32_t full[4]) {
    full[0] = full[1] = 0;
    full[2] = rows;
    full[3] = cols;
    const int32_t* w = window_or_null ? window_or_null : full;
    return window_ok(w, rows, cols) ? w : nullptr;
}

// one frame's host part for a clip call: the sources (the own frame first, then its neighbours as rsdsfm_neighbour_poses lists them) and
// their poses from the smoothed path's pose q
constexpr int kClipSourcesMax = 15;
struct ClipPlan {
    int nsrc = 0;
    int32_t src[kClipSourcesMax];
    double M[9 * kClipSourcesMax], m[3 * kClipSourcesMax];
};

// false: a pose is not finite or a listed source's scale is not finite and positive.  radius <= 7
bool clip_plan(const double* A, const double* c_, const double* A_path, const double* c_path, const double* scales, int nsources, int q, int radius, ClipPlan* plan);

// A neighbour candidate onto (d_image, d_mask) through the window: the search for the visible pre-image where the occlusion test is asked for
// and the context searches (rsdsfm_set_occlusion_search), the occlusion test where it is asked for, else the plain window render -- the public
// entry points themselves, so that they run the code they run alone
int render_candidate(rsdsfm_ctx* ctx, bool occlusion, int tol_q16, const uint8_t* d_image_n, int channels, const double* d_depth_n, const double* d_R_n, const double* d_t_n,
                     double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const double* M9, const double* m3, int id,
                     const int32_t* window, uint8_t* d_image, uint8_t* d_mask, uint8_t* d_source_or_null, int64_t* d_counts_or_null);

// The reference of a frame call: its image (channels planes), mask and source plane zeroed, then the own frame (source id 1) through the
// window; the own frame never goes through the occlusion test.  stage: the message prefix ("denoise frame")
int render_reference(rsdsfm_ctx* ctx, const char* stage, const uint8_t* d_image_n, int channels, const double* d_depth_n, const double* d_R_n, const double* d_t_n, double fx,
                     double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const double* M9, const double* m3, const int32_t* window,
                     uint8_t* d_rimage, uint8_t* d_rmask, uint8_t* d_rsource);

// A member of the dense workspace that is made when first asked for (a size change releases it with the rest)
template <class T>
inline int ensure_plane(Ctx* c, T** ptr, size_t bytes, const char* message) {
    if (!*ptr && hipMalloc(reinterpret_cast<void**>(ptr), bytes) != hipSuccess) {
        *ptr = nullptr;
        return fail(c, RSDSFM_ERR_HIP, message);
    }
    return RSDSFM_OK;
}

// The int64 counters a clip call collects on the device and hands to the host in one copy and one wait at its end
class DeviceCounts {
public:
    DeviceCounts() = default;
    ~DeviceCounts() { release(); }
    DeviceCounts(const DeviceCounts&) = delete;
    DeviceCounts& operator=(const DeviceCounts&) = delete;
    // n counters when `wanted` (else none: at() gives NULL), zeroed on the stream when `zero`
    int alloc(Ctx* c, bool wanted, size_t n, bool zero = false);
    int64_t* at(size_t i) const { return d_ ? d_ + i : nullptr; }
    explicit operator bool() const { return d_ != nullptr; }
    size_t size() const { return n_; }
    // rc: what the calls returned.  RSDSFM_OK: copy to host, wait, free; a failed copy or wait is the result.  Else: still wait and free, and rc
    int fetch(Ctx* c, int64_t* host, int rc);

private:
    void release();
    int64_t* d_ = nullptr;
    size_t n_ = 0;
};

// The clip walk of the stages that render every frame of a clip from its registered neighbours (denoise, super-resolution, clean plate).
// outputs: the arrays of per-frame output planes; [0] images and [1] masks are required, the others may be NULL.
struct ClipOutputs {
    uint8_t* const* planes[4] = {nullptr, nullptr, nullptr, nullptr};
};
// the checks of the clip's arrays, in front of the stage's own parameter check.  stage: the message prefix ("denoise video"); optional_note: what
// the refusal of a missing output says about the optional arrays ("its weight plane when the array is passed")
int clip_arrays_check(Ctx* c, const char* stage, const uint8_t* const* d_frames, int nsources, const double* const* d_depth_maps, const double* const* d_R,
                      const double* const* d_t, const double* A, const double* c_, const double* A_path, const double* c_path, const double* scales,
                      const ClipOutputs& outputs, const char* optional_note);
// one frame: its plan, the plan's sources gathered from the clip's arrays, its output planes (NULL where the array is) and its device counters
struct ClipFrame {
    const ClipPlan* plan;
    const uint8_t* img[kClipSourcesMax];
    const double *map[kClipSourcesMax], *R[kClipSourcesMax], *t[kClipSourcesMax];
    uint8_t* out[4];
    int64_t* d_counts;
};
// behind the checks: no output is a frame of the clip, then every frame's plan (a refused pose enqueues nothing)
int clip_plans(Ctx* c, const char* stage, const uint8_t* const* d_frames, int nsources, const double* A, const double* c_, const double* A_path, const double* c_path,
               const double* scales, int radius, const ClipOutputs& outputs, std::vector<ClipPlan>* plans);
// frame q of the walk
ClipFrame clip_frame(const ClipPlan& plan, const uint8_t* const* d_frames, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t,
                     const ClipOutputs& outputs, int q, int64_t* d_counts);
// the walk: the plans, then frame_call(const ClipFrame&) per frame with ncounters device counters each; counts_or_null filled by one copy and
// one wait at the end
template <class FrameCall>
int walk_clip(Ctx* c, const char* stage, const uint8_t* const* d_frames, int nsources, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t,
              const double* A, const double* c_, const double* A_path, const double* c_path, const double* scales, int radius, const ClipOutputs& outputs, int ncounters,
              int64_t* counts_or_null, FrameCall frame_call) {
    std::vector<ClipPlan> plans;
    int rc = clip_plans(c, stage, d_frames, nsources, A, c_, A_path, c_path, scales, radius, outputs, &plans);
    if (rc != RSDSFM_OK) return rc;
    DeviceCounts counts;
    rc = counts.alloc(c, counts_or_null != nullptr, (size_t)ncounters * (size_t)nsources);
    for (int q = 0; q < nsources && rc == RSDSFM_OK; ++q)
        rc = frame_call(clip_frame(plans[q], d_frames, d_depth_maps, d_R, d_t, outputs, q, counts.at((size_t)ncounters * (size_t)q)));
    return counts.fetch(c, counts_or_null, rc);
}

}  // namespace rsdsfm
