// stabilize_search_host.hip -- C ABI of the stabiliser's search for the visible pre-image (include/rsdsfm_stabilize_search.h;
// tests/stabilize_search_spec_numpy.py is the definition, stabilize_search_kernels.hip the kernels): the frame call's checks, the two planes
// it adds to the context's dense workspace on first use, and the context's knob through which the clip calls reach it
// (stabilize_fill_host.hip, stabilize_crop_host.hip, stabilize_blend_host.hip).
#include <cmath>

#include "clip_stage_host.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_search.hpp"

using namespace rsdsfm;

extern "C" {

int rsdsfm_stabilize_search_launches(int32_t rows, int32_t cols) { return rsdsfm_stabilize_window_launches(rows, cols); }

int rsdsfm_set_occlusion_search(rsdsfm_ctx* ctx, int32_t on) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    if (on != 0 && on != 1) return fail(c, RSDSFM_ERR_INVALID, "rsdsfm_set_occlusion_search: 0 (reject) or 1 (search for the visible pre-image)");
    c->occlusion_search = on;
    return RSDSFM_OK;
}

int rsdsfm_stabilize_search_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image_n, int32_t channels, const double* d_depth_n_colmajor, const double* d_R_n_rows9,
                                      const double* d_t_n_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int mode, int q5_mode,
                                      int32_t iterations, const double* M9, const double* m3, int32_t source_id, const int32_t window[4], uint8_t* d_image_inout,
                                      uint8_t* d_mask_inout, uint8_t* d_source_or_null, int32_t tol_q16, int64_t* d_counts3_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (!d_image_n || !d_depth_n_colmajor || !d_R_n_rows9 || !d_t_n_rows3 || !d_image_inout || !d_mask_inout || d_image_inout == d_image_n ||
        d_source_or_null == d_mask_inout)
        return fail(c, RSDSFM_ERR_INVALID, "null or aliased device pointer");
    if (((uintptr_t)d_image_n | (uintptr_t)d_image_inout | (uintptr_t)d_mask_inout | (uintptr_t)d_source_or_null) & 3u)
        return fail(c, RSDSFM_ERR_INVALID, "search frame: images, mask and source plane must be 4-byte aligned");
    if ((uintptr_t)d_counts3_or_null & 7u) return fail(c, RSDSFM_ERR_INVALID, "search frame: the [taken, rejected, recovered] counters must be 8-byte aligned");
    if (source_id < 1 || source_id > 255) return fail(c, RSDSFM_ERR_INVALID, "search frame: source_id must be in [1, 255] (1 is the own frame, 0 nobody)");
    if (tol_q16 < 0 || tol_q16 > kVisibleTolQ16Max) return fail(c, RSDSFM_ERR_INVALID, "search frame: tol_q16 must be in [1, 65536], or 0 for the default");
    if (!M9 || !m3 || !finite_all(M9, 9) || !finite_all(m3, 3)) return fail(c, RSDSFM_ERR_INVALID, "search frame: the pose (M, m) must be given and finite");
    if (!window_ok(window, rows, cols))
        return fail(c, RSDSFM_ERR_INVALID, "search frame: the window (r0, c0, h, w) needs h >= 1, w >= 1 and must lie inside the frame");
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);  // a size change releases the two planes with the rest
    if (rc != RSDSFM_OK) return rc;
    rc = ensure_plane(c, &ws->d_search, search_ws_bytes(rows, cols), "search frame: no memory for the key plane and the depth plane");
    if (rc != RSDSFM_OK) return rc;
    StabPose vp;
    for (int i = 0; i < 9; ++i) vp.M[i] = M9[i];
    for (int i = 0; i < 3; ++i) vp.m[i] = m3[i];
    return stabilize_search_launch(c, *ws, search_ws_layout(ws->d_search, rows, cols), d_image_n, channels, d_depth_n_colmajor, d_R_n_rows9, d_t_n_rows3, fx, fy, cx, cy,
                                   rows, cols, mode, q5_mode, iterations ? iterations : 3, vp, source_id, window, d_image_inout, d_mask_inout, d_source_or_null,
                                   tol_q16 ? tol_q16 : RSDSFM_OCCLUSION_TOL_Q16_DEFAULT, d_counts3_or_null);
}

}  // extern "C"
