// stabilize_host.hip -- C ABI of the stabiliser (include/rsdsfm_stabilize.h; tests/stabilize_spec_numpy.py is the definition,
// stabilize_kernels.hip the kernels): the path smoother and the virtual poses (host arithmetic, operation by operation the spec's), the
// frame call on the dense rectifier's workspace, and the clip call, which CALLS the public entry points one after another.
#include <cmath>
#include <vector>

#include "../../include/rsdsfm_stabilize.h"
#include "clip_stage_host.hpp"
#include "last_frame.hpp"
#include "link.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"
#include "stabilize.hpp"

namespace rsdsfm {
namespace {

rsdsfm_stabilize_params stabilize_defaults() { return rsdsfm_stabilize_params{4.0, 0, 1, (int32_t)sizeof(rsdsfm_stabilize_params), 0}; }

bool stabilize_params_ok(const rsdsfm_stabilize_params& p) {
    if (p.struct_bytes != 0 && p.struct_bytes != (int32_t)sizeof(rsdsfm_stabilize_params)) return false;
    return std::isfinite(p.sigma) && p.sigma > 0.0 && p.radius >= 0 && p.radius <= 1024 && (p.last_frame == 0 || p.last_frame == 1);
}

// mat3 and so3_log: stabilize.hpp (the retimer interpolates the path with them); finite_all: clip_stage_host.hpp

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_stabilize_params_init(rsdsfm_stabilize_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = stabilize_defaults();
    return RSDSFM_OK;
}

int rsdsfm_smooth_path(const double* A, const double* c, int32_t nframes, const rsdsfm_stabilize_params* params_or_null, double* A_s, double* c_s) {
    if (!A || !c || !A_s || !c_s || nframes < 1) return RSDSFM_ERR_INVALID;
    const rsdsfm_stabilize_params p = params_or_null ? *params_or_null : stabilize_defaults();
    if (!stabilize_params_ok(p)) return RSDSFM_ERR_INVALID;
    const int r = p.radius ? p.radius : (int)std::ceil(3.0 * p.sigma);
    for (int q = 0; q < nframes; ++q) {
        const double* Aq = A + 9 * (size_t)q;
        const double* cq = c + 3 * (size_t)q;
        double num[3] = {0.0, 0.0, 0.0}, numc[3] = {0.0, 0.0, 0.0}, den = 0.0;
        const int j0 = -r < -q ? -q : -r, j1 = r > nframes - 1 - q ? nframes - 1 - q : r;  // frames outside the clip are skipped
        for (int j = j0; j <= j1; ++j) {
            const double g = std::exp(-(double)((int64_t)j * j) / (2.0 * p.sigma * p.sigma));
            double rel[9], l[3];
            mat3(Aq, true, A + 9 * (size_t)(q + j), rel);
            so3_log(rel, l);
            const double* cj = c + 3 * (size_t)(q + j);
            for (int i = 0; i < 3; ++i) {
                num[i] = num[i] + g * l[i];
                numc[i] = numc[i] + g * (cj[i] - cq[i]);
            }
            den = den + g;
        }
        const double mean[3] = {num[0] / den, num[1] / den, num[2] / den};
        double E[9];
        link_rodrigues(mean, E);
        mat3(Aq, false, E, A_s + 9 * (size_t)q);
        for (int i = 0; i < 3; ++i) c_s[3 * (size_t)q + i] = p.translation ? cq[i] + numc[i] / den : cq[i];
    }
    return RSDSFM_OK;
}

int rsdsfm_virtual_poses(const double* A, const double* c, const double* A_s, const double* c_s, const double* scales, int32_t npairs, int32_t translation,
                         double* M, double* m) {
    if (!A || !c || !A_s || !c_s || !M || !m || npairs < 1 || (translation && !scales)) return RSDSFM_ERR_INVALID;
    if (translation)
        for (int q = 0; q < npairs; ++q)
            if (!std::isfinite(scales[q]) || !(scales[q] > 0.0)) return RSDSFM_ERR_INVALID;
    for (int q = 0; q < npairs; ++q) {
        const double* As = A_s + 9 * (size_t)q;
        mat3(As, true, A + 9 * (size_t)q, M + 9 * (size_t)q);
        const double d[3] = {c[3 * (size_t)q] - c_s[3 * (size_t)q], c[3 * (size_t)q + 1] - c_s[3 * (size_t)q + 1], c[3 * (size_t)q + 2] - c_s[3 * (size_t)q + 2]};
        for (int i = 0; i < 3; ++i)
            m[3 * (size_t)q + i] = translation ? ((As[i] * d[0] + As[3 + i] * d[1]) + As[6 + i] * d[2]) / scales[q] : 0.0;
    }
    return RSDSFM_OK;
}

int rsdsfm_stabilize_launches(int32_t rows, int32_t cols, int32_t count) {
    if (rows < 2 || cols < 2 || rows > 16384 || cols > 16384) return RSDSFM_ERR_INVALID;
    return rectify_dense_launch_count(rows, cols) + (count ? 1 : 0);
}

int rsdsfm_stabilize_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, int32_t channels, const double* d_depth_map_colmajor, const double* d_R_rows9,
                               const double* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int mode, int q5_mode,
                               int32_t iterations, const double* M9, const double* m3, uint8_t* d_image_out, uint8_t* d_mask_or_null,
                               double* d_filled_depth_or_null, float* d_disp_or_null, int64_t* d_valid_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (!d_image || !d_depth_map_colmajor || !d_R_rows9 || !d_t_rows3 || !d_image_out || d_image_out == d_image)
        return fail(c, RSDSFM_ERR_INVALID, "null or aliased device pointer");
    if (((uintptr_t)d_image | (uintptr_t)d_image_out | (uintptr_t)d_mask_or_null) & 3u)
        return fail(c, RSDSFM_ERR_INVALID, "dense rectifier: images and mask must be 4-byte aligned");
    if ((uintptr_t)d_valid_or_null & 7u) return fail(c, RSDSFM_ERR_INVALID, "stabilise: the valid counter must be 8-byte aligned");
    if (!M9 || !m3 || !finite_all(M9, 9) || !finite_all(m3, 3)) return fail(c, RSDSFM_ERR_INVALID, "stabilise: the virtual pose (M, m) must be given and finite");
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    unsigned char* d_mask = d_mask_or_null;
    if (d_valid_or_null && !d_mask) {  // a count without a caller's mask: the workspace's plane
        if (!ws->d_mask && hipMalloc(reinterpret_cast<void**>(&ws->d_mask), (size_t)rows * (size_t)cols) != hipSuccess)
            return fail(c, RSDSFM_ERR_HIP, "stabilise: no memory for the mask plane");
        d_mask = ws->d_mask;
    }
    StabPose vp;
    for (int i = 0; i < 9; ++i) vp.M[i] = M9[i];
    for (int i = 0; i < 3; ++i) vp.m[i] = m3[i];
    rc = stabilize_launch(c, *ws, d_image, channels, d_depth_map_colmajor, d_R_rows9, d_t_rows3, fx, fy, cx, cy, rows, cols, mode, q5_mode,
                          iterations ? iterations : 3, vp, d_image_out, d_mask, d_filled_depth_or_null, d_valid_or_null);
    if (rc != RSDSFM_OK) return rc;
    if (d_disp_or_null)  // the caller's float pairs need not be 8-byte aligned: the kernels keep the plane of the workspace
        RSDSFM_HIP_CHECK(c, hipMemcpyAsync(d_disp_or_null, ws->d_disp, sizeof(float2) * (size_t)rows * (size_t)cols, hipMemcpyDeviceToDevice, c->stream));
    return RSDSFM_OK;
}

int rsdsfm_stabilize_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                               double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                               const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows, double* const* d_depth_maps,
                               double* const* d_R, double* const* d_t, rsdsfm_frame_result* results,
                               const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks_or_null,
                               const rsdsfm_link_params* link_params_or_null, rsdsfm_link_record* records, double* scales, double* A, double* c_,
                               uint8_t* broken_or_null, const rsdsfm_fuse_params* fuse_params_or_null, double* const* d_fused_maps_or_null,
                               const rsdsfm_stabilize_params* stabilize_params_or_null, int mode, int q5_mode, int32_t iterations, double* A_s,
                               double* c_s, double* M, double* m, uint8_t* const* d_stab_images, uint8_t* const* d_masks_out_or_null,
                               int64_t* valid_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (nframes < 2) return fail(c, RSDSFM_ERR_INVALID, "stabilise video: nframes must be >= 2");
    const int np = nframes - 1;
    if (!d_frames || !d_flows || !d_depth_maps || !d_R || !d_t || !results || !params)
        return fail(c, RSDSFM_ERR_INVALID,
                    "stabilise video: d_flows, d_depth_maps, d_R and d_t are required -- every pair's field, map and pose table is read after the whole clip is solved");
    const int nr = stabilize_rendered_frames(stabilize_params_or_null, nframes);  // rendered frames: np, and the last frame when asked for
    if (!all_set(d_R, nr) || !all_set(d_t, nr)) return fail(c, RSDSFM_ERR_INVALID, "stabilise video: every pair needs a pose table of its own (d_R, d_t)");
    if (nr > np && (!all_set(d_depth_maps, nr) || !all_set(d_flows, np) || !scales))
        return fail(c, RSDSFM_ERR_INVALID, "stabilise video: the last frame needs a depth map of its own (d_depth_maps[nframes - 1]), the last pair's field and scales");
    if (!A_s || !c_s || !M || !m || !d_stab_images) return fail(c, RSDSFM_ERR_INVALID, "stabilise video: null pointer");
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    const rsdsfm_stabilize_params sp = stabilize_params_or_null ? *stabilize_params_or_null : stabilize_defaults();
    if (!stabilize_params_ok(sp))
        return fail(c, RSDSFM_ERR_INVALID, "rsdsfm_stabilize_params: sigma must be finite and > 0, radius in [0, 1024], last_frame 0 or 1, struct_bytes 0 or sizeof (use rsdsfm_stabilize_params_init)");
    if (!all_set(d_stab_images, nr) || (d_masks_out_or_null && !all_set(d_masks_out_or_null, nr)) || (d_fused_maps_or_null && !all_set(d_fused_maps_or_null, nr)))
        return fail(c, RSDSFM_ERR_INVALID, "stabilise video: null device pointer");
    for (int p = 0; p < nr; ++p) {
        if (d_stab_images[p] == d_frames[p]) return fail(c, RSDSFM_ERR_INVALID, "stabilise video: a pair's output image is its frame");
        if (((uintptr_t)d_stab_images[p] | (uintptr_t)d_frames[p] | (uintptr_t)(d_masks_out_or_null ? d_masks_out_or_null[p] : nullptr)) & 3u)
            return fail(c, RSDSFM_ERR_INVALID, "dense rectifier: images and mask must be 4-byte aligned");
    }
    // the solve, the links and the chain: the public entry point itself, so that it runs the code it runs alone
    rc = rsdsfm_solve_video_linked_dev(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds, d_flows,
                                       d_depth_maps, d_R, d_t, results, check_params_or_null, d_masks_or_null, link_params_or_null, records, scales, A, c_,
                                       broken_or_null, nullptr);
    if (rc != RSDSFM_OK) return rc;
    // the renderer runs on the context's stream and reads every pair's map and pose table: nothing of a lane's may still be in flight
    for (rsdsfm_ctx* lane : c->lanes) RSDSFM_HIP_CHECK(c, hipStreamSynchronize(lane->c.stream));
    if (d_fused_maps_or_null) {
        std::vector<double> v(3 * (size_t)np), w(3 * (size_t)np), k((size_t)np);
        for (int q = 0; q < np; ++q) {
            for (int i = 0; i < 3; ++i) v[3 * q + i] = results[q].v[i], w[3 * q + i] = results[q].w[i];
            k[q] = results[q].k;
        }
        rc = rsdsfm_fuse_depths_dev(ctx, d_flows, d_depth_maps, v.data(), w.data(), k.data(), np, rows, cols, fx, fy, cx, cy, gamma,
                                    params->use_global_shutter_mode ? 1 : 0, records, fuse_params_or_null, d_fused_maps_or_null, nullptr, nullptr, nullptr);
        if (rc != RSDSFM_OK) return rc;
    }
    if (nr > np) {  // the last frame: its pair's map moved onto it, its pose table from its pair's motion, its pair's unit
        const rsdsfm_frame_result& last = results[np - 1];
        const int gs = params->use_global_shutter_mode ? 1 : 0;
        rc = rsdsfm_last_frame_dev(ctx, d_flows[np - 1], d_depth_maps[np - 1], last.v, last.w, last.k, rows, cols, fx, fy, cx, cy, gamma, gs, d_depth_maps[np], d_R[np],
                                   d_t[np], nullptr, nullptr);
        if (rc == RSDSFM_OK && d_fused_maps_or_null)
            rc = rsdsfm_advance_depth_dev(ctx, d_flows[np - 1], d_fused_maps_or_null[np - 1], last.v, last.w, last.k, rows, cols, fx, fy, cx, cy, gamma, gs,
                                          d_fused_maps_or_null[np], nullptr, nullptr);
        if (rc != RSDSFM_OK) return rc;
        scales[np] = scales[np - 1];
    }
    if (rsdsfm_smooth_path(A, c_, nframes, &sp, A_s, c_s) != RSDSFM_OK) return fail(c, RSDSFM_ERR_INVALID, "stabilise video: the path smoother refused its arguments");
    if (rsdsfm_virtual_poses(A, c_, A_s, c_s, scales, nr, sp.translation, M, m) != RSDSFM_OK)
        return fail(c, RSDSFM_ERR_INVALID, "stabilise video: a pair's scale is not finite and positive");
    int64_t* d_valid = nullptr;
    if (valid_or_null) RSDSFM_HIP_CHECK(c, hipMalloc(reinterpret_cast<void**>(&d_valid), sizeof(int64_t) * (size_t)nr));
    for (int p = 0; p < nr && rc == RSDSFM_OK; ++p)
        rc = rsdsfm_stabilize_frame_dev(ctx, d_frames[p], channels, d_fused_maps_or_null ? d_fused_maps_or_null[p] : d_depth_maps[p], d_R[p], d_t[p], fx, fy, cx, cy,
                                        rows, cols, mode, q5_mode, iterations, M + 9 * (size_t)p, m + 3 * (size_t)p, d_stab_images[p],
                                        d_masks_out_or_null ? d_masks_out_or_null[p] : nullptr, nullptr, nullptr, d_valid ? d_valid + p : nullptr);
    if (d_valid) {
        hipError_t e = rc == RSDSFM_OK ? hipMemcpyAsync(valid_or_null, d_valid, sizeof(int64_t) * (size_t)nr, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        (void)hipFree(d_valid);
        if (rc == RSDSFM_OK) RSDSFM_HIP_CHECK(c, e);
    }
    return rc;
}

}  // extern "C"
