// shutter_host.hip -- C ABI of the synthetic shutter (include/rsdsfm_shutter.h; tests/shutter_spec_numpy.py is the definition,
// shutter_kernels.hip the kernel): the sub-instants (host arithmetic, operation by operation the spec's), the accumulate call, the frame
// call, which CALLS the public retime entry points per kept sub-instant and the public accumulate, and the clip call.
#include <cmath>
#include <vector>

#include "clip_stage_host.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"
#include "shutter.hpp"

namespace rsdsfm {
namespace {

rsdsfm_shutter_params shutter_defaults() {
    return rsdsfm_shutter_params{RSDSFM_SHUTTER_DEFAULT, RSDSFM_SHUTTER_SAMPLES_DEFAULT, RSDSFM_SHUTTER_MIN_SAMPLES_DEFAULT, (int32_t)sizeof(rsdsfm_shutter_params), {0, 0, 0}};
}

// the params, or the defaults for NULL; false: refused (the shutter's range against the clip is rsdsfm_shutter_times')
bool shutter_params_resolve(const rsdsfm_shutter_params* in, rsdsfm_shutter_params* out) {
    *out = in ? *in : shutter_defaults();
    if (!struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_shutter_params))) return false;
    return out->samples >= 1 && out->samples <= kShutterSamplesMax && out->min_samples >= 1 && out->min_samples <= out->samples;
}

const char* const kShutterParamsMessage =
    "rsdsfm_shutter_params: samples in [1, 64], min_samples in [1, samples], struct_bytes 0 or sizeof (use rsdsfm_shutter_params_init)";

int shutter_shape_check(Ctx* c, int channels, int rows, int cols) {
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "shutter: rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "shutter: channels must be 1 or 3");
    return RSDSFM_OK;
}

// one exposed frame's host part: the kept sub-instants and, per kept one, the sources and their poses
struct ShutterPlan {
    int kept = 0;
    int32_t src[2 * kShutterSamplesMax], nsrc[kShutterSamplesMax], wq[kShutterSamplesMax];
    double M[18 * kShutterSamplesMax], m[6 * kShutterSamplesMax];
};

bool shutter_plan(const double* A, const double* c_, const double* A_path, const double* c_path, const double* scales, int nsources, double t,
                  const rsdsfm_shutter_params& sp, ShutterPlan* plan) {
    double times[kShutterSamplesMax];
    int32_t kept = 0;
    if (rsdsfm_shutter_times(t, sp.shutter, sp.samples, nsources, times, &kept) != RSDSFM_OK) return false;
    for (int j = 0; j < kept; ++j) {
        double At[9], ct[3];
        if (rsdsfm_retime_poses(A, c_, A_path, c_path, scales, nsources, times[j], plan->src + 2 * j, plan->nsrc + j, plan->wq + j, plan->M + 18 * j, plan->m + 6 * j, At, ct) !=
            RSDSFM_OK)
            return false;
        if (!finite_all(plan->M + 18 * j, 9 * plan->nsrc[j]) || !finite_all(plan->m + 6 * j, 3 * plan->nsrc[j])) return false;
    }
    plan->kept = kept;
    return true;
}

const char* const kShutterPlanMessage =
    "shutter: t must be finite and in [0, nsources - 1], the shutter finite and in [0, nsources - 1], and the sources' poses and scales finite (scales positive)";

// what the frame and clip calls check of the clip before anything is enqueued
int shutter_clip_check(Ctx* c, const uint8_t* const* d_frames, int nsources, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t,
                       const double* A, const double* c_, const double* A_path, const double* c_path, const double* scales) {
    if (nsources < 1) return fail(c, RSDSFM_ERR_INVALID, "shutter: nsources must be >= 1");
    if (!d_frames || !d_depth_maps || !d_R || !d_t || !A || !c_ || !A_path || !c_path || !scales) return fail(c, RSDSFM_ERR_INVALID, "shutter: null array");
    if (!all_set(d_frames, nsources) || !all_set(d_depth_maps, nsources) || !all_set(d_R, nsources) || !all_set(d_t, nsources))
        return fail(c, RSDSFM_ERR_INVALID, "shutter: every source needs its frame, depth map and pose table");
    for (int n = 0; n < nsources; ++n)
        if ((uintptr_t)d_frames[n] & 3u) return fail(c, RSDSFM_ERR_INVALID, "shutter: every frame must be 4-byte aligned");
    return RSDSFM_OK;
}

// the outputs of one instant against the clip's frames
int shutter_alias_check(Ctx* c, const uint8_t* const* d_frames, int nsources, const uint8_t* d_image_out, const uint8_t* d_mask_out, const uint8_t* d_coverage) {
    for (int n = 0; n < nsources; ++n)
        if (d_frames[n] == d_image_out || d_frames[n] == d_mask_out || (d_coverage && d_frames[n] == d_coverage))
            return fail(c, RSDSFM_ERR_INVALID, "shutter: an output plane may not be a frame of the clip");
    return RSDSFM_OK;
}

// the workspace's sample planes and cells, made when first asked for
int shutter_ws(Ctx* c, int rows, int cols, DenseWs** ws) {
    const int rc = rectify_dense_ws(c, rows, cols, ws);  // a size change releases them with the rest
    if (rc != RSDSFM_OK) return rc;
    return ensure_plane(c, &(*ws)->d_shutter, shutter_ws_bytes(rows, cols), "shutter: no memory for the sample planes and the cells");
}

// the enqueues of one exposed frame (everything checked by the caller): the public calls one after another
int shutter_frame_run(rsdsfm_ctx* ctx, const ShutterPlan& plan, const uint8_t* const* d_frames, int rows, int cols, int channels, double fx, double fy, double cx, double cy,
                      const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, int mode, int q5_mode, int iterations, int min_samples,
                      const rsdsfm_retime_params* retime_or_null, const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_coverage,
                      int64_t* d_counts3) {
    Ctx* c = &ctx->c;
    DenseWs* ws = nullptr;
    int rc = shutter_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    const size_t P = blend_plane_bytes(rows, cols);
    uint8_t* smask = ws->d_shutter;
    uint8_t* simage = ws->d_shutter + P;
    uint16_t* cells = reinterpret_cast<uint16_t*>(ws->d_shutter + 4 * P);
    const int need = min_samples < plan.kept ? min_samples : plan.kept;  // a clipped window asks of a pixel what it can give
    for (int j = 0; j < plan.kept; ++j) {
        const int n0 = plan.src[2 * j], n1 = plan.nsrc[j] == 2 ? n0 + 1 : n0;
        const uint8_t* img[2] = {d_frames[n0], d_frames[n1]};
        const double* map[2] = {d_depth_maps[n0], d_depth_maps[n1]};
        const double* R[2] = {d_R[n0], d_R[n1]};
        const double* t[2] = {d_t[n0], d_t[n1]};
        rc = rsdsfm_retime_frame_dev(ctx, img, channels, map, R, t, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, plan.nsrc[j], plan.M + 18 * j, plan.m + 6 * j,
                                     plan.wq[j], retime_or_null, window_or_null, simage, smask, nullptr, nullptr);
        if (rc != RSDSFM_OK) return rc;
        rc = rsdsfm_shutter_accumulate_dev(ctx, simage, smask, channels, rows, cols, cells, j == 0, j == plan.kept - 1, plan.kept, need, d_image_out, d_mask_out, d_coverage,
                                           d_counts3);
        if (rc != RSDSFM_OK) return rc;
    }
    return RSDSFM_OK;
}

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_shutter_params_init(rsdsfm_shutter_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = shutter_defaults();
    return RSDSFM_OK;
}

int rsdsfm_shutter_times(double t, double shutter, int32_t samples, int32_t nsources, double* times_out, int32_t* nkept_out) {
    if (!times_out || !nkept_out || samples < 1 || samples > kShutterSamplesMax || nsources < 1) return RSDSFM_ERR_INVALID;
    const double last = (double)(nsources - 1);
    if (!std::isfinite(shutter) || shutter < 0.0 || shutter > last) return RSDSFM_ERR_INVALID;
    if (!std::isfinite(t) || t < 0.0 || t > last) return RSDSFM_ERR_INVALID;
    int kept = 0;
    for (int j = 0; j < samples; ++j) {
        const double u = ((double)j + 0.5) / (double)samples - 0.5;
        const double tj = t + shutter * u;
        if (tj >= 0.0 && tj <= last) times_out[kept++] = tj;
    }
    *nkept_out = kept;  // >= 1: the sub-instant nearest t on the inner side of a clipped window lies within shutter / 2 <= (nsources - 1) / 2 of t
    return RSDSFM_OK;
}

int rsdsfm_shutter_accumulate_launches(void) { return 1; }

int rsdsfm_shutter_launches(int32_t rows, int32_t cols, int32_t n_one_source, int32_t n_two_sources) {
    if (n_one_source < 0 || n_two_sources < 0 || (int64_t)n_one_source + n_two_sources < 1 || (int64_t)n_one_source + n_two_sources > kShutterSamplesMax)
        return RSDSFM_ERR_INVALID;
    const int one = rsdsfm_retime_launches(rows, cols, 1), two = rsdsfm_retime_launches(rows, cols, 2);
    if (one < 0 || two < 0) return RSDSFM_ERR_INVALID;
    return n_one_source * one + n_two_sources * two + (n_one_source + n_two_sources) * rsdsfm_shutter_accumulate_launches();
}

int rsdsfm_shutter_accumulate_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, const uint8_t* d_mask, int32_t channels, int32_t rows, int32_t cols,
                                  uint16_t* d_cells_or_null, int32_t first, int32_t last, int32_t nsamples, int32_t min_samples, uint8_t* d_image_out,
                                  uint8_t* d_mask_out, uint8_t* d_coverage_or_null, int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if ((first != 0 && first != 1) || (last != 0 && last != 1)) return fail(c, RSDSFM_ERR_INVALID, "shutter accumulate: first and last must be 0 or 1");
    if (nsamples < 1 || nsamples > kShutterSamplesMax || min_samples < 1 || min_samples > nsamples)
        return fail(c, RSDSFM_ERR_INVALID, "shutter accumulate: nsamples must be in [1, 64] and min_samples in [1, nsamples]");
    int rc = shutter_shape_check(c, channels, rows, cols);
    if (rc != RSDSFM_OK) return rc;
    if (last) {
        rc = output_planes_check(c, "shutter", {d_image_out, d_mask_out, d_coverage_or_null}, d_counts3_or_null, false);
        if (rc != RSDSFM_OK) return rc;
    } else {  // the outputs are not read
        d_image_out = d_mask_out = d_coverage_or_null = nullptr;
        d_counts3_or_null = nullptr;
    }
    if (!d_image || !d_mask || d_image == d_mask) return fail(c, RSDSFM_ERR_INVALID, "shutter accumulate: the sample needs its image and its mask");
    if (!d_cells_or_null && !(first && last)) return fail(c, RSDSFM_ERR_INVALID, "shutter accumulate: the cells may be NULL only with first and last");
    if (((uintptr_t)d_image | (uintptr_t)d_mask) & 3u) return fail(c, RSDSFM_ERR_INVALID, "shutter: every plane must be 4-byte aligned");
    if ((uintptr_t)d_cells_or_null & 7u) return fail(c, RSDSFM_ERR_INVALID, "shutter accumulate: the cells must be 8-byte aligned");
    const void* in[3] = {d_image, d_mask, d_cells_or_null};
    const void* io[3] = {d_image_out, d_mask_out, d_coverage_or_null};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3 && io[i]; ++j)
            if (in[j] == io[i]) return fail(c, RSDSFM_ERR_INVALID, "shutter accumulate: an output plane may not be the sample or the cells");
    if (d_cells_or_null && ((const void*)d_cells_or_null == d_image || (const void*)d_cells_or_null == d_mask))
        return fail(c, RSDSFM_ERR_INVALID, "shutter accumulate: the cells may not be the sample");
    return shutter_accumulate_launch(c, d_image, d_mask, channels, rows, cols, d_cells_or_null, first == 1, last == 1, nsamples, min_samples, d_image_out, d_mask_out,
                                     d_coverage_or_null, d_counts3_or_null);
}

int rsdsfm_shutter_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                             double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                             const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations, double t,
                             const rsdsfm_shutter_params* shutter_or_null, const rsdsfm_retime_params* retime_or_null, const int32_t* window_or_null,
                             uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_coverage_or_null, int64_t* d_counts3_or_null, int32_t* nkept_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_shutter_params sp;
    if (!shutter_params_resolve(shutter_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kShutterParamsMessage);
    rc = shutter_clip_check(c, d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales);
    if (rc != RSDSFM_OK) return rc;
    rc = output_planes_check(c, "shutter", {d_image_out, d_mask_out, d_coverage_or_null}, d_counts3_or_null, false);
    if (rc != RSDSFM_OK) return rc;
    rc = shutter_alias_check(c, d_frames, nsources, d_image_out, d_mask_out, d_coverage_or_null);
    if (rc != RSDSFM_OK) return rc;
    ShutterPlan plan;  // every sub-instant's sources and poses first
    if (!shutter_plan(A, c_, A_path, c_path, scales, nsources, t, sp, &plan)) return fail(c, RSDSFM_ERR_INVALID, kShutterPlanMessage);
    rc = shutter_frame_run(ctx, plan, d_frames, rows, cols, channels, fx, fy, cx, cy, d_depth_maps, d_R, d_t, mode, q5_mode, iterations, sp.min_samples, retime_or_null,
                           window_or_null, d_image_out, d_mask_out, d_coverage_or_null, d_counts3_or_null);
    if (rc == RSDSFM_OK && nkept_or_null) *nkept_or_null = plan.kept;
    return rc;
}

int rsdsfm_shutter_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                             double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                             const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                             const double* times, int32_t ntimes, const rsdsfm_shutter_params* shutter_or_null, const rsdsfm_retime_params* retime_or_null,
                             const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks, uint8_t* const* d_out_coverage_or_null,
                             int32_t* kept_out, int64_t* counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (ntimes < 1) return fail(c, RSDSFM_ERR_INVALID, "shutter video: ntimes must be >= 1");
    if (!times || !kept_out) return fail(c, RSDSFM_ERR_INVALID, "shutter video: null array");
    if (!d_out_images || !d_out_masks || !all_set(d_out_images, ntimes) || !all_set(d_out_masks, ntimes) ||
        (d_out_coverage_or_null && !all_set(d_out_coverage_or_null, ntimes)))
        return fail(c, RSDSFM_ERR_INVALID, "shutter video: every instant needs its image and its mask (and its coverage plane when the array is passed)");
    // every instant's sub-instants (rsdsfm_shutter_times, rsdsfm_retime_poses) before the first frame call: a refused time enqueues nothing.  The
    // frame call computes them again: host arithmetic, a microsecond per sample
    rsdsfm_shutter_params sp;
    if (!shutter_params_resolve(shutter_or_null, &sp)) return fail(c, RSDSFM_ERR_INVALID, kShutterParamsMessage);
    int rc = shutter_clip_check(c, d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales);
    if (rc != RSDSFM_OK) return rc;
    std::vector<int32_t> kept(ntimes);
    for (int i = 0; i < ntimes; ++i) {
        ShutterPlan plan;
        if (!shutter_plan(A, c_, A_path, c_path, scales, nsources, times[i], sp, &plan)) return fail(c, RSDSFM_ERR_INVALID, kShutterPlanMessage);
        kept[i] = plan.kept;
    }
    DeviceCounts counts;
    rc = counts.alloc(c, counts_or_null != nullptr, 3 * (size_t)ntimes);
    for (int i = 0; i < ntimes && rc == RSDSFM_OK; ++i)  // the public entry point itself, so that it runs the code it runs alone
        rc = rsdsfm_shutter_frame_dev(ctx, d_frames, nsources, rows, cols, channels, fx, fy, cx, cy, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, mode, q5_mode,
                                      iterations, times[i], shutter_or_null, retime_or_null, window_or_null, d_out_images[i], d_out_masks[i],
                                      d_out_coverage_or_null ? d_out_coverage_or_null[i] : nullptr, counts.at(3 * (size_t)i), nullptr);
    rc = counts.fetch(c, counts_or_null, rc);
    if (rc != RSDSFM_OK) return rc;
    for (int i = 0; i < ntimes; ++i) kept_out[i] = kept[i];
    return RSDSFM_OK;
}

}  // extern "C"
