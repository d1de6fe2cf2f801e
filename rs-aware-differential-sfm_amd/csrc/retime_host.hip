// retime_host.hip -- C ABI of the retimer (include/rsdsfm_retime.h; tests/retime_spec_numpy.py is the definition, retime_kernels.hip the
// kernel): the path between its poses and the sources' poses (host arithmetic, operation by operation the spec's, with the path smoother's
// helpers of stabilize.hpp), the merge call, the frame call, which CALLS the public render entry points on the context's layers, and the
// clip call, which calls the frame call per instant.
#include <cmath>
#include <cstring>
#include <vector>

#include "clip_stage_host.hpp"
#include "link.hpp"
#include "rectify_dense.hpp"
#include "retime.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"
#include "stabilize.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {
namespace {

rsdsfm_retime_params retime_defaults() {
    return rsdsfm_retime_params{RSDSFM_RETIME_THRESHOLD_DEFAULT, 0, 0, (int32_t)sizeof(rsdsfm_retime_params), {0, 0, 0, 0}};
}

// the params, or the defaults for NULL; false: refused
bool retime_params_resolve(const rsdsfm_retime_params* in, rsdsfm_retime_params* out) {
    *out = in ? *in : retime_defaults();
    if (!struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_retime_params))) return false;
    return out->threshold >= 0 && out->threshold <= kRetimeThresholdMax && occlusion_words_ok(out->occlusion, out->occlusion_tol_q16);
}

const char* const kRetimeParamsMessage =
    "rsdsfm_retime_params: threshold in [0, 255], occlusion 0 or 1, occlusion_tol_q16 in [0, 65536], struct_bytes 0 or sizeof (use rsdsfm_retime_params_init)";

// the merge's argument checks, for the merge call and, before anything is enqueued, for the frame call (whose layers are the context's: NULL here)
int retime_merge_check(Ctx* c, const uint8_t* d_image_a, const uint8_t* d_mask_a, const uint8_t* d_image_b, const uint8_t* d_mask_b, bool layers, int channels, int rows,
                       int cols, int weight_q16, int threshold, const uint8_t* d_image_out, const uint8_t* d_mask_out, const uint8_t* d_source, const int64_t* d_counts5) {
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "retime merge: rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "retime merge: channels must be 1 or 3");
    if (weight_q16 < 0 || weight_q16 > kRetimeWeightMax) return fail(c, RSDSFM_ERR_INVALID, "retime merge: weight_q16 must be in [0, 65535]");
    if (threshold < 0 || threshold > kRetimeThresholdMax) return fail(c, RSDSFM_ERR_INVALID, "retime merge: threshold must be in [0, 255]");
    if (!d_image_out || !d_mask_out) return fail(c, RSDSFM_ERR_INVALID, "retime merge: null output plane");
    if (layers) {
        if (!d_image_a || !d_mask_a) return fail(c, RSDSFM_ERR_INVALID, "retime merge: null layer");
        if ((d_image_b == nullptr) != (d_mask_b == nullptr)) return fail(c, RSDSFM_ERR_INVALID, "retime merge: layer b needs its image and its mask, or neither");
        if (!d_mask_b && weight_q16 != 0) return fail(c, RSDSFM_ERR_INVALID, "retime merge: without layer b the weight must be 0");
    }
    const uint8_t* in[4] = {d_image_a, d_mask_a, d_image_b, d_mask_b};
    const uint8_t* io[3] = {d_image_out, d_mask_out, d_source};
    for (int i = 0; i < 3; ++i) {
        if (!io[i]) continue;
        for (int j = 0; j < 4; ++j)
            if (in[j] == io[i]) return fail(c, RSDSFM_ERR_INVALID, "retime merge: an output plane may not be a layer");
        for (int j = 0; j < i; ++j)
            if (io[j] == io[i]) return fail(c, RSDSFM_ERR_INVALID, "retime merge: the output planes must be distinct");
    }
    if (((uintptr_t)d_image_a | (uintptr_t)d_mask_a | (uintptr_t)d_image_b | (uintptr_t)d_mask_b | (uintptr_t)d_image_out | (uintptr_t)d_mask_out | (uintptr_t)d_source) & 3u)
        return fail(c, RSDSFM_ERR_INVALID, "retime merge: every plane must be 4-byte aligned");
    if ((uintptr_t)d_counts5 & 7u) return fail(c, RSDSFM_ERR_INVALID, "retime merge: the counters must be 8-byte aligned");
    return RSDSFM_OK;
}

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_retime_params_init(rsdsfm_retime_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = retime_defaults();
    return RSDSFM_OK;
}

int rsdsfm_path_at(const double* A_path, const double* c_path, int32_t nposes, double t, double* A_t9, double* c_t3) {
    if (!A_path || !c_path || !A_t9 || !c_t3 || nposes < 1) return RSDSFM_ERR_INVALID;
    if (!std::isfinite(t) || t < 0.0 || t > (double)(nposes - 1)) return RSDSFM_ERR_INVALID;
    const double fl = std::floor(t), tau = t - fl;
    const int q = (int)fl;
    const double* Aq = A_path + 9 * (size_t)q;
    const double* cq = c_path + 3 * (size_t)q;
    if (tau == 0.0) {  // the entry's bytes
        std::memcpy(A_t9, Aq, 9 * sizeof(double));
        std::memcpy(c_t3, cq, 3 * sizeof(double));
        return RSDSFM_OK;
    }
    double rel[9], l[3], E[9];
    mat3(Aq, true, Aq + 9, rel);
    so3_log(rel, l);
    const double step[3] = {tau * l[0], tau * l[1], tau * l[2]};
    link_rodrigues(step, E);
    mat3(Aq, false, E, A_t9);
    for (int i = 0; i < 3; ++i) c_t3[i] = cq[i] + tau * (cq[3 + i] - cq[i]);
    return RSDSFM_OK;
}

int rsdsfm_retime_poses(const double* A, const double* c, const double* A_path, const double* c_path, const double* scales, int32_t nsources, double t,
                        int32_t src_out[2], int32_t* nsrc_out, int32_t* weight_q16_out, double* M_out, double* m_out, double* A_t9, double* c_t3) {
    if (!A || !c || !A_path || !c_path || !scales || !src_out || !nsrc_out || !weight_q16_out || !M_out || !m_out || !A_t9 || !c_t3 || nsources < 1)
        return RSDSFM_ERR_INVALID;
    if (!std::isfinite(t) || t < 0.0 || t > (double)(nsources - 1)) return RSDSFM_ERR_INVALID;
    const double fl = std::floor(t), tau = t - fl;
    const int n0 = (int)fl, nsrc = tau > 0.0 ? 2 : 1;
    for (int k = 0; k < nsrc; ++k)  // nothing is written when a listed source's scale is refused
        if (!std::isfinite(scales[n0 + k]) || !(scales[n0 + k] > 0.0)) return RSDSFM_ERR_INVALID;
    const int rc = rsdsfm_path_at(A_path, c_path, nsources, t, A_t9, c_t3);
    if (rc != RSDSFM_OK) return rc;
    for (int k = 0; k < nsrc; ++k) {
        const int n = n0 + k;
        pose_from(A_t9, c_t3, A + 9 * (size_t)n, c + 3 * (size_t)n, scales[n], M_out + 9 * (size_t)k, m_out + 3 * (size_t)k);
    }
    src_out[0] = n0;
    src_out[1] = nsrc == 2 ? n0 + 1 : -1;
    *nsrc_out = nsrc;
    int w = 0;
    if (nsrc == 2) {
        w = (int)std::rint(tau * 65536.0);
        w = w < 1 ? 1 : w > kRetimeWeightMax ? kRetimeWeightMax : w;
    }
    *weight_q16_out = w;
    return RSDSFM_OK;
}

int rsdsfm_retime_merge_launches(void) { return 1; }

int rsdsfm_retime_launches(int32_t rows, int32_t cols, int32_t nsrc) {
    if (nsrc != 1 && nsrc != 2) return RSDSFM_ERR_INVALID;
    const int one = rsdsfm_stabilize_window_launches(rows, cols);
    return one < 0 ? one : nsrc * one + 1;
}

int rsdsfm_retime_merge_dev(rsdsfm_ctx* ctx, const uint8_t* d_image_a, const uint8_t* d_mask_a, const uint8_t* d_image_b_or_null, const uint8_t* d_mask_b_or_null,
                            int32_t channels, int32_t rows, int32_t cols, int32_t weight_q16, int32_t threshold, uint8_t* d_image_out, uint8_t* d_mask_out,
                            uint8_t* d_source_or_null, int64_t* d_counts5_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    const int rc = retime_merge_check(c, d_image_a, d_mask_a, d_image_b_or_null, d_mask_b_or_null, true, channels, rows, cols, weight_q16, threshold, d_image_out,
                                      d_mask_out, d_source_or_null, d_counts5_or_null);
    if (rc != RSDSFM_OK) return rc;
    return retime_merge_launch(c, d_image_a, d_mask_a, d_image_b_or_null, d_mask_b_or_null, channels, rows, cols, weight_q16, threshold, d_image_out, d_mask_out,
                               d_source_or_null, d_counts5_or_null);
}

int rsdsfm_retime_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                            const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                            int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M18, const double* m6, int32_t weight_q16,
                            const rsdsfm_retime_params* params_or_null, const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out,
                            uint8_t* d_source_or_null, int64_t* d_counts5_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc != 1 && nsrc != 2) return fail(c, RSDSFM_ERR_INVALID, "retime frame: nsrc must be 1 or 2");
    if (nsrc == 1 && weight_q16 != 0) return fail(c, RSDSFM_ERR_INVALID, "retime frame: with one source the weight must be 0");
    rsdsfm_retime_params rp;
    if (!retime_params_resolve(params_or_null, &rp)) return fail(c, RSDSFM_ERR_INVALID, kRetimeParamsMessage);
    rc = frame_sources_check(c, "retime frame", d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, nsrc, {d_image_out});  // the image output alone (DESIGN's known gaps)
    if (rc == RSDSFM_OK) rc = frame_poses_check(c, "retime frame", M18, m6, nsrc);
    if (rc == RSDSFM_OK)
        rc = retime_merge_check(c, nullptr, nullptr, nullptr, nullptr, false, channels, rows, cols, weight_q16, rp.threshold, d_image_out, d_mask_out, d_source_or_null,
                                d_counts5_or_null);
    int32_t full[4];
    const int32_t* window = nullptr;
    if (rc == RSDSFM_OK) rc = frame_window(c, "retime frame", window_or_null, rows, cols, full, &window);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);  // a size change releases the layers with the rest
    if (rc != RSDSFM_OK) return rc;
    rc = ensure_plane(c, &ws->d_layer, blend_layer_bytes(rows, cols), "retime frame: no memory for layer A");
    if (rc == RSDSFM_OK && nsrc == 2) rc = ensure_plane(c, &ws->d_layer2, retime_layer2_bytes(rows, cols), "retime frame: no memory for layer B");
    if (rc != RSDSFM_OK) return rc;
    const RenderGeom g{channels, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations};
    const BlendLayer a = blend_layer(ws->d_layer, rows, cols);
    uint8_t* lmask[2] = {a.mask, nsrc == 2 ? ws->d_layer2 : nullptr};
    uint8_t* limage[2] = {a.image, nsrc == 2 ? ws->d_layer2 + blend_plane_bytes(rows, cols) : nullptr};
    for (int k = 0; k < nsrc; ++k) {
        rc = render_layer(ctx, "retime frame: zeroing a layer failed", rp.occlusion == 1, rp.occlusion_tol_q16, source_view(d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, k), g,
                          M18 + 9 * k, m6 + 3 * k, k == 0 ? RSDSFM_RETIME_FROM_A : RSDSFM_RETIME_FROM_B, window, limage[k], lmask[k]);
        if (rc != RSDSFM_OK) return rc;
    }
    // the public entry point itself, so that it runs the code it runs alone
    return rsdsfm_retime_merge_dev(ctx, limage[0], lmask[0], limage[1], lmask[1], channels, rows, cols, weight_q16, rp.threshold, d_image_out, d_mask_out, d_source_or_null,
                                   d_counts5_or_null);
}

int rsdsfm_retime_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                            double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                            const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                            const double* times, int32_t ntimes, const rsdsfm_retime_params* params_or_null, const int32_t* window_or_null,
                            uint8_t* const* d_out_images, uint8_t* const* d_out_masks, uint8_t* const* d_out_sources_or_null, int32_t* sources_out,
                            int32_t* weights_out, int64_t* counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (nsources < 1 || ntimes < 1) return fail(c, RSDSFM_ERR_INVALID, "retime video: nsources and ntimes must be >= 1");
    if (!d_frames || !d_depth_maps || !d_R || !d_t || !A || !c_ || !A_path || !c_path || !scales || !times || !sources_out || !weights_out)
        return fail(c, RSDSFM_ERR_INVALID, "retime video: null array");
    if (!all_set(d_frames, nsources) || !all_set(d_depth_maps, nsources) || !all_set(d_R, nsources) || !all_set(d_t, nsources))
        return fail(c, RSDSFM_ERR_INVALID, "retime video: every source needs its frame, depth map and pose table");
    if (!d_out_images || !d_out_masks || !all_set(d_out_images, ntimes) || !all_set(d_out_masks, ntimes) ||
        (d_out_sources_or_null && !all_set(d_out_sources_or_null, ntimes)))
        return fail(c, RSDSFM_ERR_INVALID, "retime video: every instant needs its image and its mask (and its source plane when the array is passed)");
    // every instant's sources and poses first: a refused time enqueues nothing
    std::vector<int32_t> src(2 * (size_t)ntimes), nsrc(ntimes), wq(ntimes);
    std::vector<double> M(18 * (size_t)ntimes), m(6 * (size_t)ntimes);
    for (int i = 0; i < ntimes; ++i) {
        double At[9], ct[3];
        if (rsdsfm_retime_poses(A, c_, A_path, c_path, scales, nsources, times[i], &src[2 * (size_t)i], &nsrc[i], &wq[i], &M[18 * (size_t)i], &m[6 * (size_t)i], At, ct) !=
            RSDSFM_OK)
            return fail(c, RSDSFM_ERR_INVALID, "retime video: a time must be finite and in [0, nsources - 1], and its sources' scales finite and positive");
    }
    DeviceCounts counts;
    int rc = counts.alloc(c, counts_or_null != nullptr, 5 * (size_t)ntimes);
    for (int i = 0; i < ntimes && rc == RSDSFM_OK; ++i) {
        const int n0 = src[2 * (size_t)i], n1 = nsrc[i] == 2 ? n0 + 1 : n0;
        const uint8_t* img[2] = {d_frames[n0], d_frames[n1]};
        const double* map[2] = {d_depth_maps[n0], d_depth_maps[n1]};
        const double* R[2] = {d_R[n0], d_R[n1]};
        const double* t[2] = {d_t[n0], d_t[n1]};
        rc = rsdsfm_retime_frame_dev(ctx, img, channels, map, R, t, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, nsrc[i], &M[18 * (size_t)i], &m[6 * (size_t)i],
                                     wq[i], params_or_null, window_or_null, d_out_images[i], d_out_masks[i], d_out_sources_or_null ? d_out_sources_or_null[i] : nullptr,
                                     counts.at(5 * (size_t)i));
    }
    rc = counts.fetch(c, counts_or_null, rc);
    if (rc != RSDSFM_OK) return rc;
    for (int i = 0; i < ntimes; ++i) {
        sources_out[2 * (size_t)i] = src[2 * (size_t)i];
        sources_out[2 * (size_t)i + 1] = src[2 * (size_t)i + 1];
        weights_out[i] = wq[i];
    }
    return RSDSFM_OK;
}

}  // extern "C"
