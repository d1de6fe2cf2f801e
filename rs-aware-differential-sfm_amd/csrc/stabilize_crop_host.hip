// stabilize_crop_host.hip -- C ABI of the stabiliser's crop and zoom (include/rsdsfm_stabilize_crop.h; tests/stabilize_crop_spec_numpy.py is
// the definition, stabilize_crop_kernels.hip the kernels): the window search on the context's dense workspace, which waits for one 8-byte
// copy and decodes the winner's key here, the frame call, and the clip call, which CALLS the public entry points one after another.
#include <cmath>
#include <vector>

#include "../../include/rsdsfm_stabilize_crop.h"
#include "clip_stage_host.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "last_frame.hpp"
#include "sequence_host.hpp"
#include "stabilize_crop.hpp"
#include "stabilize_search.hpp"
#include "stabilize_visible.hpp"

namespace rsdsfm {
namespace {

constexpr int kCropMarginDefault = 1, kCropMarginMax = 64;
constexpr int kCropFillRadiusDefault = 2, kCropFillRadiusMax = 16;  // the border fill's

rsdsfm_stabilize_crop_params crop_defaults() {
    return rsdsfm_stabilize_crop_params{0, kCropMarginDefault, (int32_t)sizeof(rsdsfm_stabilize_crop_params), {0, 0, 0, 0}};
}

bool crop_params_ok(const rsdsfm_stabilize_crop_params& p, int rows, int cols) {
    if (p.struct_bytes != 0 && p.struct_bytes != (int32_t)sizeof(rsdsfm_stabilize_crop_params)) return false;
    return p.margin >= 0 && p.margin <= kCropMarginMax && p.max_empty >= 0 && p.max_empty <= (int64_t)rows * cols;
}

}  // namespace

CropWs crop_ws_layout(void* d_crop) {
    char* b = static_cast<char*>(d_crop);
    return CropWs{reinterpret_cast<unsigned long long*>(b), reinterpret_cast<const unsigned char**>(b + 8),
                  reinterpret_cast<unsigned*>(b + 8 + sizeof(void*) * (size_t)kCropPlanesMax)};
}

size_t crop_ws_bytes(int rows, int cols) { return 8 + sizeof(void*) * (size_t)kCropPlanesMax + sizeof(unsigned) * (size_t)(rows + 1) * (size_t)(cols + 1); }

void crop_decode_key(unsigned long long key, int rows, int cols, int32_t window[4]) {
    window[0] = window[1] = window[2] = window[3] = 0;
    if (!key) return;
    const int64_t h = (int64_t)(key >> 45);
    window[0] = 16383 - (int32_t)((key >> 14) & 16383u);
    window[1] = 16383 - (int32_t)(key & 16383u);
    window[2] = (int32_t)h;
    window[3] = (int32_t)((h * cols) / rows);
}

}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_stabilize_crop_params_init(rsdsfm_stabilize_crop_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = crop_defaults();
    return RSDSFM_OK;
}

int rsdsfm_crop_window_launches(int32_t rows, int32_t cols) {
    if (!frame_size_ok(rows, cols)) return RSDSFM_ERR_INVALID;
    return 3;
}

int rsdsfm_stabilize_window_launches(int32_t rows, int32_t cols) { return rsdsfm_stabilize_fill_launches(rows, cols); }

int rsdsfm_crop_window_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_masks, int32_t nmasks, int32_t rows, int32_t cols,
                           const rsdsfm_stabilize_crop_params* params_or_null, int32_t window_out[4]) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "crop window: rows and cols must be in [2, 16384]");
    if (!window_out || nmasks < 1 || nmasks > kCropPlanesMax || !all_set(d_masks, nmasks))
        return fail(c, RSDSFM_ERR_INVALID, "crop window: 1 .. 4096 mask planes and window_out are required");
    for (int k = 0; k < nmasks; ++k)
        if ((uintptr_t)d_masks[k] & 3u) return fail(c, RSDSFM_ERR_INVALID, "crop window: every mask plane must be 4-byte aligned");
    const rsdsfm_stabilize_crop_params cp = params_or_null ? *params_or_null : crop_defaults();
    if (!crop_params_ok(cp, rows, cols))
        return fail(c, RSDSFM_ERR_INVALID,
                    "rsdsfm_stabilize_crop_params: margin in [0, 64], max_empty in [0, rows cols], struct_bytes 0 or sizeof (use rsdsfm_stabilize_crop_params_init)");
    DenseWs* ws = nullptr;
    int rc = rectify_dense_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    rc = ensure_plane(c, &ws->d_crop, crop_ws_bytes(rows, cols), "crop window: no memory for the summed-area table");
    if (rc != RSDSFM_OK) return rc;
    const CropWs cw = crop_ws_layout(ws->d_crop);
    unsigned long long key = 0;
    // the planes' pointers go behind whatever the stream still runs on the table; this call waits below, so `d_masks` is read in time
    hipError_t e = hipMemcpyAsync(cw.d_planes, d_masks, sizeof(void*) * (size_t)nmasks, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        rc = crop_window_launch(c, cw, nmasks, rows, cols, cp.max_empty, cp.margin);
        if (rc == RSDSFM_OK) e = hipMemcpyAsync(&key, cw.d_key, sizeof(key), hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (rc != RSDSFM_OK) return rc;
    RSDSFM_HIP_CHECK(c, e);
    RSDSFM_HIP_CHECK(c, es);
    crop_decode_key(key, rows, cols, window_out);
    return RSDSFM_OK;
}

int rsdsfm_stabilize_window_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image_n, int32_t channels, const double* d_depth_n_colmajor, const double* d_R_n_rows9,
                                      const double* d_t_n_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols, int mode, int q5_mode,
                                      int32_t iterations, const double* M9, const double* m3, int32_t source_id, const int32_t window[4], uint8_t* d_image_inout,
                                      uint8_t* d_mask_inout, uint8_t* d_source_or_null, int64_t* d_filled_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (!d_image_n || !d_depth_n_colmajor || !d_R_n_rows9 || !d_t_n_rows3 || !d_image_inout || !d_mask_inout || d_image_inout == d_image_n ||
        d_source_or_null == d_mask_inout)
        return fail(c, RSDSFM_ERR_INVALID, "null or aliased device pointer");
    if (((uintptr_t)d_image_n | (uintptr_t)d_image_inout | (uintptr_t)d_mask_inout | (uintptr_t)d_source_or_null) & 3u)
        return fail(c, RSDSFM_ERR_INVALID, "window frame: images, mask and source plane must be 4-byte aligned");
    if ((uintptr_t)d_filled_or_null & 7u) return fail(c, RSDSFM_ERR_INVALID, "window frame: the filled counter must be 8-byte aligned");
    if (source_id < 1 || source_id > 255) return fail(c, RSDSFM_ERR_INVALID, "window frame: source_id must be in [1, 255] (1 is the own frame, 0 nobody)");
    if (!M9 || !m3 || !finite_all(M9, 9) || !finite_all(m3, 3)) return fail(c, RSDSFM_ERR_INVALID, "window frame: the pose (M, m) must be given and finite");
    if (!window_ok(window, rows, cols))
        return fail(c, RSDSFM_ERR_INVALID, "window frame: the window (r0, c0, h, w) needs h >= 1, w >= 1 and must lie inside the frame");
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    StabPose vp;
    for (int i = 0; i < 9; ++i) vp.M[i] = M9[i];
    for (int i = 0; i < 3; ++i) vp.m[i] = m3[i];
    return stabilize_window_launch(c, *ws, d_image_n, channels, d_depth_n_colmajor, d_R_n_rows9, d_t_n_rows3, fx, fy, cx, cy, rows, cols, mode, q5_mode,
                                   iterations ? iterations : 3, vp, source_id, window, d_image_inout, d_mask_inout, d_source_or_null, d_filled_or_null);
}

int rsdsfm_stabilize_video_cropped_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                       double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                       const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows, double* const* d_depth_maps,
                                       double* const* d_R, double* const* d_t, rsdsfm_frame_result* results,
                                       const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks_or_null,
                                       const rsdsfm_link_params* link_params_or_null, rsdsfm_link_record* records, double* scales, double* A, double* c_,
                                       uint8_t* broken_or_null, const rsdsfm_fuse_params* fuse_params_or_null, double* const* d_fused_maps_or_null,
                                       const rsdsfm_stabilize_params* stabilize_params_or_null, int mode, int q5_mode, int32_t iterations, double* A_s,
                                       double* c_s, double* M, double* m, uint8_t* const* d_stab_images, uint8_t* const* d_masks_out,
                                       int64_t* valid_or_null, const rsdsfm_stabilize_fill_params* fill_params_or_null, uint8_t* const* d_sources_or_null,
                                       int64_t* counts_or_null, const rsdsfm_stabilize_crop_params* crop_params_or_null, const int32_t* window_in_or_null,
                                       uint8_t* const* d_crop_images, uint8_t* const* d_crop_masks, uint8_t* const* d_crop_sources_or_null,
                                       int32_t window_out[4], int64_t* crop_counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (nframes < 2) return fail(c, RSDSFM_ERR_INVALID, "stabilise video: nframes must be >= 2");
    const int np = stabilize_rendered_frames(stabilize_params_or_null, nframes);  // rendered frames: the pairs' first frames, and the last frame when asked for
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "crop: rows and cols must be in [2, 16384]");
    if (fill_params_or_null && ((fill_params_or_null->struct_bytes != 0 && fill_params_or_null->struct_bytes != (int32_t)sizeof(rsdsfm_stabilize_fill_params)) ||
                                fill_params_or_null->radius < 0 || fill_params_or_null->radius > kCropFillRadiusMax || !visible_words_ok(fill_params_or_null)))
        return fail(c, RSDSFM_ERR_INVALID,
                    "rsdsfm_stabilize_fill_params: radius in [0, 16], occlusion 0 or 1, occlusion_tol_q16 in [0, 65536], struct_bytes 0 or sizeof (use rsdsfm_stabilize_fill_params_init)");
    const bool occ = visible_asked(fill_params_or_null);  // the neighbours go through the occlusion test: [taken, rejected] per frame call, the first is the count
    const bool srch = search_asked(c, fill_params_or_null);  // ... and through the search for the visible pre-image: [taken, rejected, recovered]
    const int cw = candidate_counters(occ, srch);
    const int radius = fill_params_or_null ? fill_params_or_null->radius : kCropFillRadiusDefault;  // 0 here: no fill at all
    const rsdsfm_stabilize_crop_params cp = crop_params_or_null ? *crop_params_or_null : crop_defaults();
    if (!crop_params_ok(cp, rows, cols))
        return fail(c, RSDSFM_ERR_INVALID,
                    "rsdsfm_stabilize_crop_params: margin in [0, 64], max_empty in [0, rows cols], struct_bytes 0 or sizeof (use rsdsfm_stabilize_crop_params_init)");
    if (window_in_or_null && !window_ok(window_in_or_null, rows, cols))
        return fail(c, RSDSFM_ERR_INVALID, "crop: window_in (r0, c0, h, w) needs h >= 1, w >= 1 and must lie inside the frame");
    if (!window_out || !all_set(d_crop_images, np) || !all_set(d_crop_masks, np) || (d_crop_sources_or_null && !all_set(d_crop_sources_or_null, np)))
        return fail(c, RSDSFM_ERR_INVALID, "crop: window_out, d_crop_images and d_crop_masks are required");
    if (!all_set(d_masks_out, np)) return fail(c, RSDSFM_ERR_INVALID, "crop: d_masks_out is required -- the window is found from the masks");
    for (int p = 0; p < np; ++p) {
        const uint8_t* src = d_crop_sources_or_null ? d_crop_sources_or_null[p] : nullptr;
        if (((uintptr_t)d_crop_images[p] | (uintptr_t)d_crop_masks[p] | (uintptr_t)src) & 3u)
            return fail(c, RSDSFM_ERR_INVALID, "crop: crop images, masks and source planes must be 4-byte aligned");
        if (src == d_crop_masks[p]) return fail(c, RSDSFM_ERR_INVALID, "crop: a source plane may not be the mask");
    }
    // the inner clip: the public entry point itself, so that it runs the code it runs alone
    int rc;
    if (radius == 0) {
        std::vector<int64_t> own;
        int64_t* valid = valid_or_null;
        if (counts_or_null && !valid) {
            own.resize((size_t)np);
            valid = own.data();
        }
        rc = rsdsfm_stabilize_video_dev(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds, d_flows, d_depth_maps,
                                        d_R, d_t, results, check_params_or_null, d_masks_or_null, link_params_or_null, records, scales, A, c_, broken_or_null,
                                        fuse_params_or_null, d_fused_maps_or_null, stabilize_params_or_null, mode, q5_mode, iterations, A_s, c_s, M, m, d_stab_images,
                                        d_masks_out, valid);
        if (rc == RSDSFM_OK && counts_or_null)
            for (int p = 0; p < np; ++p) {
                counts_or_null[2 * (size_t)p] = (int64_t)rows * cols - valid[p];
                counts_or_null[2 * (size_t)p + 1] = valid[p];
            }
    } else {
        rc = rsdsfm_stabilize_video_filled_dev(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds, d_flows,
                                               d_depth_maps, d_R, d_t, results, check_params_or_null, d_masks_or_null, link_params_or_null, records, scales, A, c_,
                                               broken_or_null, fuse_params_or_null, d_fused_maps_or_null, stabilize_params_or_null, mode, q5_mode, iterations, A_s, c_s,
                                               M, m, d_stab_images, d_masks_out, valid_or_null, fill_params_or_null, d_sources_or_null, counts_or_null);
    }
    if (rc != RSDSFM_OK) return rc;
    if (window_in_or_null) {
        for (int i = 0; i < 4; ++i) window_out[i] = window_in_or_null[i];
    } else {
        rc = rsdsfm_crop_window_dev(ctx, d_masks_out, np, rows, cols, &cp, window_out);
        if (rc != RSDSFM_OK) return rc;
    }
    const size_t plane = (size_t)rows * (size_t)cols;
    const int slots = 1 + 2 * radius;  // a counter per frame and source id, at id - 1; a skipped offset keeps its 0
    const bool have = window_out[2] >= 1;
    DeviceCounts counts;
    rc = counts.alloc(c, crop_counts_or_null && have, (size_t)np * slots * cw, true);
    if (rc != RSDSFM_OK) return rc;
    int32_t frames[2 * kCropFillRadiusMax], ids[2 * kCropFillRadiusMax], listed = 0;
    double nM[9 * 2 * kCropFillRadiusMax], nm[3 * 2 * kCropFillRadiusMax];
    for (int p = 0; p < np && rc == RSDSFM_OK; ++p) {
        uint8_t* src = d_crop_sources_or_null ? d_crop_sources_or_null[p] : nullptr;
        if (hipMemsetAsync(d_crop_images[p], 0, plane * (size_t)channels, c->stream) != hipSuccess || hipMemsetAsync(d_crop_masks[p], 0, plane, c->stream) != hipSuccess ||
            (src && hipMemsetAsync(src, 0, plane, c->stream) != hipSuccess))
            rc = fail(c, RSDSFM_ERR_HIP, "crop: zeroing the crop planes failed");
        if (!have || rc != RSDSFM_OK) continue;
        const double* map = d_fused_maps_or_null ? d_fused_maps_or_null[p] : d_depth_maps[p];
        rc = rsdsfm_stabilize_window_frame_dev(ctx, d_frames[p], channels, map, d_R[p], d_t[p], fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, M + 9 * (size_t)p,
                                               m + 3 * (size_t)p, 1, window_out, d_crop_images[p], d_crop_masks[p], src, counts.at((size_t)p * slots * cw));
        listed = 0;
        if (rc == RSDSFM_OK && radius > 0 && rsdsfm_neighbour_poses(A, c_, A_s, c_s, scales, np, p, radius, frames, ids, nM, nm, &listed) != RSDSFM_OK)
            rc = fail(c, RSDSFM_ERR_INVALID, "crop: a neighbour's scale is not finite and positive");
        for (int k = 0; k < listed && rc == RSDSFM_OK; ++k) {
            const int n = frames[k];
            const double* nmap = d_fused_maps_or_null ? d_fused_maps_or_null[n] : d_depth_maps[n];
            rc = render_candidate(ctx, occ, occ ? fill_params_or_null->occlusion_tol_q16 : 0, d_frames[n], channels, nmap, d_R[n], d_t[n], fx, fy, cx, cy, rows, cols, mode,
                                  q5_mode, iterations, nM + 9 * (size_t)k, nm + 3 * (size_t)k, ids[k], window_out, d_crop_images[p], d_crop_masks[p], src,
                                  counts.at(((size_t)p * slots + (ids[k] - 1)) * cw));
        }
    }
    if (crop_counts_or_null && !have && rc == RSDSFM_OK) {
        for (int p = 0; p < np; ++p) {
            int64_t* row = crop_counts_or_null + (size_t)p * (1 + slots);
            row[0] = (int64_t)plane;
            for (int k = 0; k < slots; ++k) row[1 + k] = 0;
        }
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    }
    if (counts) {
        std::vector<int64_t> taken(counts.size());
        rc = counts.fetch(c, taken.data(), rc);
        if (rc == RSDSFM_OK)
            for (int p = 0; p < np; ++p) {
                int64_t* row = crop_counts_or_null + (size_t)p * (1 + slots);
                int64_t sum = 0;
                for (int k = 0; k < slots; ++k) sum += (row[1 + k] = candidate_count(&taken[((size_t)p * slots + k) * cw], srch));
                row[0] = (int64_t)plane - sum;
            }
    }
    return rc;
}

}  // extern "C"
