// clip_stage_host.hip -- clip_stage_host.hpp's out-of-line part: the front of a frame call, one frame's plan, the render choice, the neighbour step, the accumulate calls' check, the device counters and the clip walk.
#include "clip_stage_host.hpp"

#include <string>
#include <vector>

#include "../../include/rsdsfm_denoise.h"
#include "../../include/rsdsfm_retime.h"
#include "../../include/rsdsfm_stabilize_crop.h"
#include "../../include/rsdsfm_stabilize_fill.h"
#include "../../include/rsdsfm_stabilize_search.h"
#include "../../include/rsdsfm_stabilize_visible.h"
#include "sequence_host.hpp"

namespace rsdsfm {

namespace {

int fail_at(Ctx* c, int code, const char* stage, const char* what) { return fail(c, code, (std::string(stage) + ": " + what).c_str()); }

}  // namespace

bool clip_plan(const double* A, const double* c_, const double* A_path, const double* c_path, const double* scales, int nsources, int q, int radius, ClipPlan* plan) {
    int32_t src2[2], nsrc = 0, wq = 0, ids[kClipSourcesMax - 1], count = 0;
    double M18[18], m6[6], At[9], ct[3];
    if (rsdsfm_retime_poses(A, c_, A_path, c_path, scales, nsources, (double)q, src2, &nsrc, &wq, M18, m6, At, ct) != RSDSFM_OK || nsrc != 1) return false;
    plan->src[0] = q;
    for (int k = 0; k < 9; ++k) plan->M[k] = M18[k];
    for (int k = 0; k < 3; ++k) plan->m[k] = m6[k];
    if (nsources > 1 && rsdsfm_neighbour_poses(A, c_, A_path, c_path, scales, nsources, q, radius, plan->src + 1, ids, plan->M + 9, plan->m + 3, &count) != RSDSFM_OK)
        return false;
    plan->nsrc = 1 + count;
    return finite_all(plan->M, 9 * plan->nsrc) && finite_all(plan->m, 3 * plan->nsrc);
}

int frame_sources_check(Ctx* c, const char* stage, const uint8_t* const* images, const double* const* depths, const double* const* R, const double* const* t, int nsrc,
                        std::initializer_list<const void*> outputs) {
    if (!images || !depths || !R || !t) return fail_at(c, RSDSFM_ERR_INVALID, stage, "null source array");
    for (int k = 0; k < nsrc; ++k) {
        bool bad = !images[k] || !depths[k] || !R[k] || !t[k] || ((uintptr_t)images[k] & 3u);
        for (const void* o : outputs) bad = bad || (o && o == (const void*)images[k]);
        if (bad) return fail_at(c, RSDSFM_ERR_INVALID, stage, "null, misaligned or aliased source pointer");
    }
    return RSDSFM_OK;
}

int frame_poses_check(Ctx* c, const char* stage, const double* M, const double* m, int nsrc) {
    if (!M || !m || !finite_all(M, 9 * nsrc) || !finite_all(m, 3 * nsrc)) return fail_at(c, RSDSFM_ERR_INVALID, stage, "the poses (M, m) must be given and finite");
    return RSDSFM_OK;
}

int output_planes_check(Ctx* c, const char* stage, std::initializer_list<const void*> planes, const int64_t* d_counts, bool counts_distinct) {
    const void* const* p = planes.begin();
    const int n = (int)planes.size();
    if (!p[0] || !p[1]) return fail_at(c, RSDSFM_ERR_INVALID, stage, "null output plane");
    uintptr_t bits = 0;
    for (int i = 0; i < n; ++i) {
        bits |= (uintptr_t)p[i];
        for (int j = i + 1; j < n; ++j)
            if (p[i] && p[i] == p[j]) return fail_at(c, RSDSFM_ERR_INVALID, stage, "the output planes must be distinct");
        if (counts_distinct && p[i] && p[i] == (const void*)d_counts) return fail_at(c, RSDSFM_ERR_INVALID, stage, "the output planes must be distinct");
    }
    if (bits & 3u) return fail_at(c, RSDSFM_ERR_INVALID, stage, "every plane must be 4-byte aligned");
    if ((uintptr_t)d_counts & 7u) return fail_at(c, RSDSFM_ERR_INVALID, stage, "the counters must be 8-byte aligned");
    return RSDSFM_OK;
}

int frame_window(Ctx* c, const char* stage, const int32_t* window_or_null, int rows, int cols, int32_t full[4], const int32_t** window) {
    *window = window_or_full(window_or_null, rows, cols, full);
    if (!*window) return fail_at(c, RSDSFM_ERR_INVALID, stage, "the window (r0, c0, h, w) needs h >= 1, w >= 1 and must lie inside the frame");
    return RSDSFM_OK;
}

int render_candidate(rsdsfm_ctx* ctx, bool occlusion, int tol_q16, const SourceView& src, const RenderGeom& g, const double* M9, const double* m3, int id,
                     const int32_t* window, uint8_t* d_image, uint8_t* d_mask, uint8_t* d_source_or_null, int64_t* d_counts_or_null) {
    if (occlusion && ctx->c.occlusion_search == 1)
        return rsdsfm_stabilize_search_frame_dev(ctx, src.image, g.channels, src.depth, src.R, src.t, g.fx, g.fy, g.cx, g.cy, g.rows, g.cols, g.mode, g.q5_mode, g.iterations, M9, m3,
                                                 id, window, d_image, d_mask, d_source_or_null, tol_q16, d_counts_or_null);
    if (occlusion)
        return rsdsfm_stabilize_visible_frame_dev(ctx, src.image, g.channels, src.depth, src.R, src.t, g.fx, g.fy, g.cx, g.cy, g.rows, g.cols, g.mode, g.q5_mode, g.iterations, M9, m3,
                                                  id, window, d_image, d_mask, d_source_or_null, tol_q16, d_counts_or_null);
    return rsdsfm_stabilize_window_frame_dev(ctx, src.image, g.channels, src.depth, src.R, src.t, g.fx, g.fy, g.cx, g.cy, g.rows, g.cols, g.mode, g.q5_mode, g.iterations, M9, m3, id,
                                             window, d_image, d_mask, d_source_or_null, d_counts_or_null);
}

int render_reference(rsdsfm_ctx* ctx, const char* stage, const SourceView& src, const RenderGeom& g, const double* M9, const double* m3, const int32_t* window,
                     uint8_t* d_rimage, uint8_t* d_rmask, uint8_t* d_rsource) {
    Ctx* c = &ctx->c;
    const size_t plane = (size_t)g.rows * (size_t)g.cols;
    if (hipMemsetAsync(d_rimage, 0, plane * (size_t)g.channels, c->stream) != hipSuccess || hipMemsetAsync(d_rmask, 0, plane, c->stream) != hipSuccess ||
        hipMemsetAsync(d_rsource, 0, plane, c->stream) != hipSuccess)
        return fail_at(c, RSDSFM_ERR_HIP, stage, "zeroing the reference failed");
    return render_candidate(ctx, false, 0, src, g, M9, m3, 1, window, d_rimage, d_rmask, d_rsource, nullptr);
}

int render_layer(rsdsfm_ctx* ctx, const char* zero_failed, bool occlusion, int tol_q16, const SourceView& src, const RenderGeom& g, const double* M9, const double* m3, int id,
                 const int32_t* window, uint8_t* d_limage, uint8_t* d_lmask) {
    Ctx* c = &ctx->c;
    const size_t plane = (size_t)g.rows * (size_t)g.cols;
    if (hipMemsetAsync(d_limage, 0, plane * (size_t)g.channels, c->stream) != hipSuccess || hipMemsetAsync(d_lmask, 0, plane, c->stream) != hipSuccess)
        return fail(c, RSDSFM_ERR_HIP, zero_failed);
    return render_candidate(ctx, occlusion, tol_q16, src, g, M9, m3, id, window, d_limage, d_lmask, nullptr, nullptr);
}

int neighbour_step(rsdsfm_ctx* ctx, const char* zero_failed, bool occlusion, int tol_q16, const SourceView& src, const RenderGeom& g, const double* M9, const double* m3,
                   const int32_t* window, const uint8_t* d_rimage, const uint8_t* d_rsource, uint8_t* d_limage, uint8_t* d_lmask, uint64_t* d_record) {
    const int rc = render_layer(ctx, zero_failed, occlusion, tol_q16, src, g, M9, m3, 2, window, d_limage, d_lmask);
    if (rc != RSDSFM_OK) return rc;
    return rsdsfm_seam_overlap_sums_dev(ctx, d_rimage, d_rsource, d_limage, d_lmask, g.channels, g.rows, g.cols, d_record);
}

int accumulate_check(Ctx* c, const char* stage, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_layer_image, const uint8_t* d_layer_mask, int channels,
                     int rows, int cols, const uint16_t* d_cells, std::initializer_list<const void*> records, int first, int last, AccumulateOutputs* out) {
    const auto refuse = [&](const char* what) { return fail_at(c, RSDSFM_ERR_INVALID, (std::string(stage) + " accumulate").c_str(), what); };
    const bool one = records.size() == 1;
    if ((first != 0 && first != 1) || (last != 0 && last != 1)) return refuse("first and last must be 0 or 1");
    if (!frame_size_ok(rows, cols)) return fail_at(c, RSDSFM_ERR_INVALID, stage, "rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail_at(c, RSDSFM_ERR_INVALID, stage, "channels must be 1 or 3");
    if (last) {
        const int rc = output_planes_check(c, stage, {out->image, out->mask, out->weight}, out->counts, false);
        if (rc != RSDSFM_OK) return rc;
    } else {  // the outputs are not read
        *out = AccumulateOutputs{nullptr, nullptr, nullptr, nullptr};
    }
    if (!d_ref_image || !d_ref_mask || d_ref_image == d_ref_mask) return refuse("the reference needs its image and its mask");
    if ((d_layer_image == nullptr) != (d_layer_mask == nullptr)) return refuse("the layer needs its image and its mask, or neither");
    if (!d_layer_image && !(first && last)) return refuse("without a layer first and last must both be 1");
    if (d_layer_image && (d_layer_image == d_layer_mask || d_layer_image == d_ref_image || d_layer_image == d_ref_mask || d_layer_mask == d_ref_image || d_layer_mask == d_ref_mask))
        return refuse("the reference's and the layer's planes must be distinct");
    if (!d_cells && !(first && last)) return refuse("the cells may be NULL only with first and last");
    const void* in[8] = {d_ref_image, d_ref_mask, d_layer_image, d_layer_mask, d_cells};  // the planes, the cells, then the records (three at most)
    int nin = 5;
    for (const void* r : records) in[nin++] = r;
    if (((uintptr_t)in[0] | (uintptr_t)in[1] | (uintptr_t)in[2] | (uintptr_t)in[3]) & 3u) return fail_at(c, RSDSFM_ERR_INVALID, stage, "every plane must be 4-byte aligned");
    for (int j = 4; j < nin; ++j)
        if ((uintptr_t)in[j] & 7u) return refuse(one ? "the cells and the record must be 8-byte aligned" : "the cells and the records must be 8-byte aligned");
    const void* io[4] = {out->image, out->mask, out->weight, out->counts};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < nin && io[i]; ++j)
            if (in[j] == io[i]) return refuse(one ? "an output may not be an input, the record or the cells" : "an output may not be an input, a record or the cells");
    for (int j = 0; j < (one ? 4 : nin) && d_cells; ++j)
        if (j != 4 && in[j] == (const void*)d_cells) return refuse(one ? "the cells may not be an input plane" : "the cells may not be an input plane or a record");
    return RSDSFM_OK;
}

int DeviceCounts::alloc(Ctx* c, bool wanted, size_t n, bool zero) {
    if (!wanted) return RSDSFM_OK;
    RSDSFM_HIP_CHECK(c, hipMalloc(reinterpret_cast<void**>(&d_), sizeof(int64_t) * n));
    n_ = n;
    if (zero) {
        const hipError_t e = hipMemsetAsync(d_, 0, sizeof(int64_t) * n, c->stream);
        if (e != hipSuccess) {
            release();
            RSDSFM_HIP_CHECK(c, e);
        }
    }
    return RSDSFM_OK;
}

int DeviceCounts::fetch(Ctx* c, int64_t* host, int rc) {
    if (!d_) return rc;
    hipError_t e = rc == RSDSFM_OK ? hipMemcpyAsync(host, d_, sizeof(int64_t) * n_, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    release();
    if (rc == RSDSFM_OK) RSDSFM_HIP_CHECK(c, e);
    return rc;
}

void DeviceCounts::release() {
    if (d_) (void)hipFree(d_);
    d_ = nullptr;
    n_ = 0;
}

int clip_arrays_check(Ctx* c, const char* stage, const uint8_t* const* d_frames, int nsources, const double* const* d_depth_maps, const double* const* d_R,
                      const double* const* d_t, const double* A, const double* c_, const double* A_path, const double* c_path, const double* scales,
                      const ClipOutputs& outputs, const char* optional_note) {
    if (nsources < 1) return fail_at(c, RSDSFM_ERR_INVALID, stage, "nsources must be >= 1");
    if (!d_frames || !d_depth_maps || !d_R || !d_t || !A || !c_ || !A_path || !c_path || !scales) return fail_at(c, RSDSFM_ERR_INVALID, stage, "null array");
    if (!all_set(d_frames, nsources) || !all_set(d_depth_maps, nsources) || !all_set(d_R, nsources) || !all_set(d_t, nsources))
        return fail_at(c, RSDSFM_ERR_INVALID, stage, "every source needs its frame, depth map and pose table");
    bool given = all_set(outputs.planes[0], nsources) && all_set(outputs.planes[1], nsources);
    for (int k = 2; k < 4; ++k) given = given && (!outputs.planes[k] || all_set(outputs.planes[k], nsources));
    if (!given) return fail_at(c, RSDSFM_ERR_INVALID, stage, (std::string("every frame needs its image and its mask (and ") + optional_note + ")").c_str());
    return RSDSFM_OK;
}

int clip_plans(Ctx* c, const char* stage, const uint8_t* const* d_frames, int nsources, const double* A, const double* c_, const double* A_path, const double* c_path,
               const double* scales, int radius, const ClipOutputs& outputs, std::vector<ClipPlan>* plans) {
    for (int q = 0; q < nsources; ++q)  // an output may not be a frame of the clip: a later frame call still reads it
        for (int n = 0; n < nsources; ++n)
            for (int k = 0; k < 4; ++k)
                if (outputs.planes[k] && d_frames[n] == outputs.planes[k][q]) return fail_at(c, RSDSFM_ERR_INVALID, stage, "an output plane may not be a frame of the clip");
    // every frame's sources and poses first: a refused pose enqueues nothing
    plans->resize(nsources);
    for (int q = 0; q < nsources; ++q)
        if (!clip_plan(A, c_, A_path, c_path, scales, nsources, q, radius, &(*plans)[q]))
            return fail_at(c, RSDSFM_ERR_INVALID, stage, "the poses must be finite and every listed source's scale finite and positive");
    return RSDSFM_OK;
}

ClipFrame clip_frame(const ClipPlan& plan, const uint8_t* const* d_frames, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t,
                     const ClipOutputs& outputs, int q, int64_t* d_counts) {
    ClipFrame f;
    f.plan = &plan;
    for (int k = 0; k < plan.nsrc; ++k) {
        const int n = plan.src[k];
        f.img[k] = d_frames[n];
        f.map[k] = d_depth_maps[n];
        f.R[k] = d_R[n];
        f.t[k] = d_t[n];
    }
    for (int k = 0; k < 4; ++k) f.out[k] = outputs.planes[k] ? outputs.planes[k][q] : nullptr;
    f.d_counts = d_counts;
    return f;
}

}  // namespace rsdsfm
