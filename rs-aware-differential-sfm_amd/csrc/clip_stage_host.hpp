// clip_stage_host.hpp -- what the hosts of the image stages behind the stabiliser share (retime, shutter, denoise, super-resolution, clean
// plate, and the fill, crop, blend and inpaint clip calls): the small argument checks, the front of a frame call (its sources, poses, outputs and
// window), one frame's sources and poses (ClipPlan), the render geometry, the three-way choice of the render entry point for a neighbour
// candidate, the neighbour step, the device counters of a clip call, and the clip walk of the stages that render
// every frame from its registered neighbours.  Helpers that report take the stage's message prefix.  DESIGN section 12, "Shared tile toolkit
// and clip walk".
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <initializer_list>
#include <vector>

#include "rsdsfm_internal.hpp"
#include "stabilize_visible.hpp"

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

// What every render of a frame call shares, filled once behind rectify_dense_check, and one source of its four arrays
struct RenderGeom {
    int channels;
    double fx, fy, cx, cy;
    int rows, cols, mode, q5_mode, iterations;
};
struct SourceView {
    const uint8_t* image;
    const double *depth, *R, *t;
};
inline SourceView source_view(const uint8_t* const* images, const double* const* depths, const double* const* R, const double* const* t, int k) {
    return SourceView{images[k], depths[k], R[k], t[k]};
}

// The front of a frame call, check by check; each refuses with RSDSFM_ERR_INVALID and "<stage>: <what>" and enqueues nothing.
// The four source arrays given, and every source given, its image 4-byte aligned and none of `outputs` (NULL entries are skipped)
int frame_sources_check(Ctx* c, const char* stage, const uint8_t* const* images, const double* const* depths, const double* const* R, const double* const* t, int nsrc,
                        std::initializer_list<const void*> outputs);
// The poses given and finite
int frame_poses_check(Ctx* c, const char* stage, const double* M, const double* m, int nsrc);
// The output planes: the first two required, the given ones distinct and 4-byte aligned, the counters 8-byte aligned; counts_distinct: the
// counters may not be one of the planes either (the plate and the erase; DESIGN's known gaps)
int output_planes_check(Ctx* c, const char* stage, std::initializer_list<const void*> planes, const int64_t* d_counts, bool counts_distinct);
// The caller's window or the whole frame (window_or_full) into *window
int frame_window(Ctx* c, const char* stage, const int32_t* window_or_null, int rows, int cols, int32_t full[4], const int32_t** window);
// The two words every *_params_resolve repeats
inline bool struct_bytes_ok(int32_t struct_bytes, size_t size) { return struct_bytes == 0 || struct_bytes == (int32_t)size; }
inline bool occlusion_words_ok(int occlusion, int tol_q16) { return (occlusion == 0 || occlusion == 1) && tol_q16 >= 0 && tol_q16 <= kVisibleTolQ16Max; }

// A neighbour candidate onto (d_image, d_mask) through the window: the search for the visible pre-image where the occlusion test is asked for
// and the context searches (rsdsfm_set_occlusion_search), the occlusion test where it is asked for, else the plain window render -- the public
// entry points themselves, with flat arguments, so that they run the code they run alone
int render_candidate(rsdsfm_ctx* ctx, bool occlusion, int tol_q16, const SourceView& src, const RenderGeom& g, const double* M9, const double* m3, int id,
                     const int32_t* window, uint8_t* d_image, uint8_t* d_mask, uint8_t* d_source_or_null, int64_t* d_counts_or_null);
// the same for the clip loops that hold no RenderGeom (the crop's and the blend's)
inline int render_candidate(rsdsfm_ctx* ctx, bool occlusion, int tol_q16, const uint8_t* d_image_n, int channels, const double* d_depth_n, const double* d_R_n, const double* d_t_n,
                            double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const double* M9, const double* m3, int id,
                            const int32_t* window, uint8_t* d_image, uint8_t* d_mask, uint8_t* d_source_or_null, int64_t* d_counts_or_null) {
    return render_candidate(ctx, occlusion, tol_q16, SourceView{d_image_n, d_depth_n, d_R_n, d_t_n}, RenderGeom{channels, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations}, M9,
                            m3, id, window, d_image, d_mask, d_source_or_null, d_counts_or_null);
}

// The reference of a frame call: its image (channels planes), mask and source plane zeroed, then the own frame (source id 1) through the
// window; the own frame never goes through the occlusion test.  stage: the message prefix ("denoise frame")
int render_reference(rsdsfm_ctx* ctx, const char* stage, const SourceView& src, const RenderGeom& g, const double* M9, const double* m3, const int32_t* window,
                     uint8_t* d_rimage, uint8_t* d_rmask, uint8_t* d_rsource);

// A neighbour onto a layer: the layer's image and mask zeroed on the stream, then render_candidate without a source plane (the id is not
// written anywhere).  zero_failed: the whole text of the RSDSFM_ERR_HIP refusal, which differs between the stages
int render_layer(rsdsfm_ctx* ctx, const char* zero_failed, bool occlusion, int tol_q16, const SourceView& src, const RenderGeom& g, const double* M9, const double* m3, int id,
                 const int32_t* window, uint8_t* d_limage, uint8_t* d_lmask);
// One neighbour of a frame call: render_layer with id 2, then the overlap record of the reference against the layer (rsdsfm_seam_overlap_sums_dev)
int neighbour_step(rsdsfm_ctx* ctx, const char* zero_failed, bool occlusion, int tol_q16, const SourceView& src, const RenderGeom& g, const double* M9, const double* m3,
                   const int32_t* window, const uint8_t* d_rimage, const uint8_t* d_rsource, uint8_t* d_limage, uint8_t* d_lmask, uint64_t* d_record);

// The checks the denoise's and the deblur's accumulate calls share ("<stage> accumulate: ...", "<stage>: ..."): first and last, the size, the
// outputs when `last` (else they are not read, and *out is cleared), the reference, the layer, the cells, the alignments, and no output an
// input.  records: the 8-byte records the call reads, one (the denoise: "the record") or more (the deblur: "a record"; the cells may then not
// be one either)
struct AccumulateOutputs {
    uint8_t *image, *mask, *weight;
    int64_t* counts;
};
int accumulate_check(Ctx* c, const char* stage, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image, const uint8_t* d_layer_mask, int channels,
                     int rows, int cols, const uint16_t* d_cells, std::initializer_list<const void*> records, int first, int last, AccumulateOutputs* out);

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
