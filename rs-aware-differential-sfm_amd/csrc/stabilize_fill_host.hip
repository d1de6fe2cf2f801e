// stabilize_fill_host.hip -- C ABI of the stabiliser's border fill (include/rsdsfm_stabilize_fill.h; tests/stabilize_fill_spec_numpy.py is
// the definition, stabilize_fill_kernels.hip the kernels): the candidates of a frame and their poses (host arithmetic, operation by
// operation the spec's), the frame call on the dense rectifier's workspace, and the clip call, which CALLS the public entry points one
// after another.
#include <cmath>
#include <vector>

#include "../../include/rsdsfm_stabilize_fill.h"
#include "clip_stage_host.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "last_frame.hpp"
#include "sequence_host.hpp"
#include "stabilize_fill.hpp"
#include "stabilize_search.hpp"
#include "stabilize_visible.hpp"

namespace rsdsfm {
namespace {

constexpr int kFillRadiusDefault = 2, kFillRadiusMax = 16;

rsdsfm_stabilize_fill_params fill_defaults() { return rsdsfm_stabilize_fill_params{kFillRadiusDefault, (int32_t)sizeof(rsdsfm_stabilize_fill_params), 0, 0}; }

bool fill_params_ok(const rsdsfm_stabilize_fill_params& p) {
    if (p.struct_bytes != 0 && p.struct_bytes != (int32_t)sizeof(rsdsfm_stabilize_fill_params)) return false;
    return p.radius >= 0 && p.radius <= kFillRadiusMax && visible_words_ok(&p);
}

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_stabilize_fill_params_init(rsdsfm_stabilize_fill_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = fill_defaults();
    return RSDSFM_OK;
}

int rsdsfm_neighbour_poses(const double* A, const double* c, const double* A_s, const double* c_s, const double* scales, int32_t npairs, int32_t q,
                           int32_t radius, int32_t* frames_out, int32_t* source_ids_out, double* M_out, double* m_out, int32_t* count_out) {
    if (!A || !c || !A_s || !c_s || !scales || !frames_out || !source_ids_out || !M_out || !m_out || !count_out) return RSDSFM_ERR_INVALID;
    if (npairs < 1 || q < 0 || q > npairs - 1 || radius < 1 || radius > kFillRadiusMax) return RSDSFM_ERR_INVALID;
    for (int d = 1; d <= radius; ++d)  // nothing is written when a listed neighbour's scale is refused
        for (int s = -1; s <= 1; s += 2) {
            const int n = q + s * d;
            if (n >= 0 && n <= npairs - 1 && (!std::isfinite(scales[n]) || !(scales[n] > 0.0))) return RSDSFM_ERR_INVALID;
        }
    const double* As = A_s + 9 * (size_t)q;
    const double* cs = c_s + 3 * (size_t)q;
    int k = 0;
    for (int d = 1; d <= radius; ++d)
        for (int s = -1; s <= 1; s += 2) {  // nearer first, previous before next
            const int n = q + s * d;
            if (n < 0 || n > npairs - 1) continue;
            pose_from(As, cs, A + 9 * (size_t)n, c + 3 * (size_t)n, scales[n], M_out + 9 * (size_t)k, m_out + 3 * (size_t)k);  // stabilize.hpp; the retimer's too
            frames_out[k] = n;
            source_ids_out[k] = 2 * d + (s > 0 ? 1 : 0);
            ++k;
        }
    *count_out = k;
    return RSDSFM_OK;
}

int rsdsfm_stabilize_fill_launches(int32_t rows, int32_t cols) {
    if (!frame_size_ok(rows, cols)) return RSDSFM_ERR_INVALID;
    return rectify_dense_launch_count(rows, cols);
}

int rsdsfm_stabilize_fill_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image_n, int32_t channels, const double* d_depth_n_colmajor, const double* d_R_n_rows9,
                                    const double* d_t_n_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int mode, int q5_mode,
                                    int32_t iterations, const double* M9, const double* m3, int32_t source_id, uint8_t* d_image_inout, uint8_t* d_mask_inout,
                                    uint8_t* d_source_or_null, int64_t* d_filled_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (!d_image_n || !d_depth_n_colmajor || !d_R_n_rows9 || !d_t_n_rows3 || !d_image_inout || !d_mask_inout || d_image_inout == d_image_n ||
        d_source_or_null == d_mask_inout)
        return fail(c, RSDSFM_ERR_INVALID, "null or aliased device pointer");
    if (((uintptr_t)d_image_n | (uintptr_t)d_image_inout | (uintptr_t)d_mask_inout | (uintptr_t)d_source_or_null) & 3u)
        return fail(c, RSDSFM_ERR_INVALID, "border fill: images, mask and source plane must be 4-byte aligned");
    if ((uintptr_t)d_filled_or_null & 7u) return fail(c, RSDSFM_ERR_INVALID, "border fill: the filled counter must be 8-byte aligned");
    if (source_id < 2 || source_id > 255) return fail(c, RSDSFM_ERR_INVALID, "border fill: source_id must be in [2, 255] (1 is the own frame, 0 nobody)");
    if (!M9 || !m3 || !finite_all(M9, 9) || !finite_all(m3, 3)) return fail(c, RSDSFM_ERR_INVALID, "border fill: the pose (M, m) must be given and finite");
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    StabPose vp;
    for (int i = 0; i < 9; ++i) vp.M[i] = M9[i];
    for (int i = 0; i < 3; ++i) vp.m[i] = m3[i];
    return stabilize_fill_launch(c, *ws, d_image_n, channels, d_depth_n_colmajor, d_R_n_rows9, d_t_n_rows3, fx, fy, cx, cy, rows, cols, mode, q5_mode,
                                 iterations ? iterations : 3, vp, source_id, d_image_inout, d_mask_inout, d_source_or_null, d_filled_or_null);
}

int rsdsfm_stabilize_video_filled_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                      double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                      const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows, double* const* d_depth_maps,
                                      double* const* d_R, double* const* d_t, rsdsfm_frame_result* results,
                                      const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks_or_null,
                                      const rsdsfm_link_params* link_params_or_null, rsdsfm_link_record* records, double* scales, double* A, double* c_,
                                      uint8_t* broken_or_null, const rsdsfm_fuse_params* fuse_params_or_null, double* const* d_fused_maps_or_null,
                                      const rsdsfm_stabilize_params* stabilize_params_or_null, int mode, int q5_mode, int32_t iterations, double* A_s,
                                      double* c_s, double* M, double* m, uint8_t* const* d_stab_images, uint8_t* const* d_masks_out,
                                      int64_t* valid_or_null, const rsdsfm_stabilize_fill_params* fill_params_or_null, uint8_t* const* d_sources_or_null,
                                      int64_t* counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (nframes < 2) return fail(c, RSDSFM_ERR_INVALID, "stabilise video: nframes must be >= 2");
    const int np = stabilize_rendered_frames(stabilize_params_or_null, nframes);  // rendered frames: the pairs' first frames, and the last frame when asked for
    const rsdsfm_stabilize_fill_params fp = fill_params_or_null ? *fill_params_or_null : fill_defaults();
    if (!fill_params_ok(fp))
        return fail(c, RSDSFM_ERR_INVALID, "rsdsfm_stabilize_fill_params: radius in [0, 16], occlusion 0 or 1, occlusion_tol_q16 in [0, 65536], struct_bytes 0 or sizeof (use rsdsfm_stabilize_fill_params_init)");
    const int radius = fp.radius ? fp.radius : kFillRadiusDefault;
    const bool occ = visible_asked(&fp);  // the candidates go through the occlusion test: [taken, rejected] per candidate, the first is the count
    const bool srch = search_asked(c, &fp);  // ... and through the search for the visible pre-image: [taken, rejected, recovered]
    const int cw = candidate_counters(occ, srch);
    const int32_t full[4] = {0, 0, rows, cols};
    if (!all_set(d_masks_out, np)) return fail(c, RSDSFM_ERR_INVALID, "border fill: d_masks_out is required -- a candidate is taken where the mask is 0");
    if (d_sources_or_null) {
        if (!all_set(d_sources_or_null, np)) return fail(c, RSDSFM_ERR_INVALID, "border fill: null device pointer");
        for (int p = 0; p < np; ++p)
            if (((uintptr_t)d_sources_or_null[p] & 3u) || d_sources_or_null[p] == d_masks_out[p])
                return fail(c, RSDSFM_ERR_INVALID, "border fill: a source plane must be 4-byte aligned and may not be the mask");
    }
    // the stabilised clip: the public entry point itself, so that it runs the code it runs alone.  The `own` column is its valid count
    std::vector<int64_t> own;
    int64_t* valid = valid_or_null;
    if (counts_or_null && !valid) {
        own.resize((size_t)np);
        valid = own.data();
    }
    int rc = rsdsfm_stabilize_video_dev(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds, d_flows, d_depth_maps,
                                        d_R, d_t, results, check_params_or_null, d_masks_or_null, link_params_or_null, records, scales, A, c_, broken_or_null,
                                        fuse_params_or_null, d_fused_maps_or_null, stabilize_params_or_null, mode, q5_mode, iterations, A_s, c_s, M, m, d_stab_images,
                                        d_masks_out, valid);
    if (rc != RSDSFM_OK) return rc;
    const size_t plane = (size_t)rows * (size_t)cols;
    const int slots = 2 * radius;
    DeviceCounts counts;  // a counter per frame and offset, at source id - 2; a skipped offset keeps its 0
    rc = counts.alloc(c, counts_or_null != nullptr, (size_t)np * slots * cw, true);
    if (rc != RSDSFM_OK) return rc;
    int32_t frames[2 * kFillRadiusMax], ids[2 * kFillRadiusMax], listed = 0;
    double nM[9 * 2 * kFillRadiusMax], nm[3 * 2 * kFillRadiusMax];
    for (int p = 0; p < np && rc == RSDSFM_OK; ++p) {
        if (d_sources_or_null && hipMemcpyAsync(d_sources_or_null[p], d_masks_out[p], plane, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            rc = fail(c, RSDSFM_ERR_HIP, "border fill: the copy of the mask to the source plane failed");
        if (rc == RSDSFM_OK && rsdsfm_neighbour_poses(A, c_, A_s, c_s, scales, np, p, radius, frames, ids, nM, nm, &listed) != RSDSFM_OK)
            rc = fail(c, RSDSFM_ERR_INVALID, "border fill: a neighbour's scale is not finite and positive");
        for (int k = 0; k < listed && rc == RSDSFM_OK; ++k) {
            const int n = frames[k];
            const double* map = d_fused_maps_or_null ? d_fused_maps_or_null[n] : d_depth_maps[n];
            uint8_t* src = d_sources_or_null ? d_sources_or_null[p] : nullptr;
            int64_t* cnt = counts.at(((size_t)p * slots + (ids[k] - 2)) * cw);
            rc = srch ? rsdsfm_stabilize_search_frame_dev(ctx, d_frames[n], channels, map, d_R[n], d_t[n], fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations,
                                                          nM + 9 * (size_t)k, nm + 3 * (size_t)k, ids[k], full, d_stab_images[p], d_masks_out[p], src,
                                                          fp.occlusion_tol_q16, cnt)
                 : occ ? rsdsfm_stabilize_visible_frame_dev(ctx, d_frames[n], channels, map, d_R[n], d_t[n], fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations,
                                                          nM + 9 * (size_t)k, nm + 3 * (size_t)k, ids[k], full, d_stab_images[p], d_masks_out[p], src,
                                                          fp.occlusion_tol_q16, cnt)
                     : rsdsfm_stabilize_fill_frame_dev(ctx, d_frames[n], channels, map, d_R[n], d_t[n], fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations,
                                                       nM + 9 * (size_t)k, nm + 3 * (size_t)k, ids[k], d_stab_images[p], d_masks_out[p], src, cnt);
        }
    }
    if (counts) {
        std::vector<int64_t> filled(counts.size());
        rc = counts.fetch(c, filled.data(), rc);
        if (rc == RSDSFM_OK)
            for (int p = 0; p < np; ++p) {
                int64_t* row = counts_or_null + (size_t)p * (2 + slots);
                int64_t rest = valid[p];
                row[1] = valid[p];
                for (int k = 0; k < slots; ++k) rest += (row[2 + k] = candidate_count(&filled[((size_t)p * slots + k) * cw], srch));
                row[0] = (int64_t)plane - rest;
            }
    }
    return rc;
}

}  // extern "C"
