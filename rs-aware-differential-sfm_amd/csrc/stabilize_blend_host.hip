// stabilize_blend_host.hip -- C ABI of the stabiliser's seam blend (include/rsdsfm_stabilize_blend.h; tests/stabilize_blend_spec_numpy.py is
// the definition, stabilize_blend_kernels.hip the kernels): the distance call and the layer call, which only enqueue, the host's gains, and
// the clip call, which CALLS the public entry points one after another on planes of the context's dense workspace.
#include <vector>

#include "../../include/rsdsfm_stabilize_blend.h"
#include "clip_stage_host.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "last_frame.hpp"
#include "sequence_host.hpp"
#include "stabilize_blend.hpp"
#include "stabilize_search.hpp"
#include "stabilize_visible.hpp"

namespace rsdsfm {
namespace {

constexpr int kBlendFillRadiusDefault = 2, kBlendFillRadiusMax = 16;  // the border fill's, as the crop's clip call admits them

rsdsfm_stabilize_blend_params blend_defaults() {
    return rsdsfm_stabilize_blend_params{kMinOverlapDefault, kFeatherDefault, 0, (int32_t)sizeof(rsdsfm_stabilize_blend_params), {0, 0, 0}};
}

// the params with every 0 replaced by its default; false: refused
bool blend_params_resolve(const rsdsfm_stabilize_blend_params* in, rsdsfm_stabilize_blend_params* out) {
    *out = in ? *in : blend_defaults();
    if (!struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_stabilize_blend_params))) return false;
    if (out->feather == 0) out->feather = kFeatherDefault;
    if (out->min_overlap == 0) out->min_overlap = kMinOverlapDefault;
    return out->feather >= 1 && out->feather <= kFeatherMax && out->min_overlap >= 0 && (out->gain_mode == 0 || out->gain_mode == 1);
}

const char* const kBlendParamsMessage =
    "rsdsfm_stabilize_blend_params: feather in [1, 64] or 0, gain_mode 0 or 1, min_overlap >= 0, struct_bytes 0 or sizeof (use rsdsfm_stabilize_blend_params_init)";

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_stabilize_blend_params_init(rsdsfm_stabilize_blend_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = blend_defaults();
    return RSDSFM_OK;
}

int rsdsfm_seam_distance_launches(int32_t rows, int32_t cols) { return frame_size_ok(rows, cols) ? 2 : RSDSFM_ERR_INVALID; }

int rsdsfm_seam_blend_layer_launches(int32_t rows, int32_t cols) { return frame_size_ok(rows, cols) ? 2 : RSDSFM_ERR_INVALID; }

int rsdsfm_seam_gains(const uint64_t* sums8, int32_t channels, int64_t min_overlap, int32_t gain_mode, uint32_t gains_out[3]) {
    if (!sums8 || !gains_out || (channels != 1 && channels != 3) || min_overlap < 0 || (gain_mode != 0 && gain_mode != 1)) return RSDSFM_ERR_INVALID;
    unsigned long long s[8];
    for (int i = 0; i < 8; ++i) s[i] = sums8[i];
    for (int c = 0; c < 3; ++c) gains_out[c] = c < channels ? seam_gain(s, channels, c, min_overlap ? min_overlap : kMinOverlapDefault, gain_mode) : kGainOne;
    return RSDSFM_OK;
}

int rsdsfm_seam_distance_dev(rsdsfm_ctx* ctx, const uint8_t* d_mask, int32_t rows, int32_t cols, int32_t feather, uint8_t* d_dist_out) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "seam distance: rows and cols must be in [2, 16384]");
    if (feather < 0 || feather > kFeatherMax) return fail(c, RSDSFM_ERR_INVALID, "seam distance: feather must be in [1, 64] (0: the default, 16)");
    if (!d_mask || !d_dist_out || d_mask == d_dist_out) return fail(c, RSDSFM_ERR_INVALID, "seam distance: null or aliased device pointer");
    if (((uintptr_t)d_mask | (uintptr_t)d_dist_out) & 3u) return fail(c, RSDSFM_ERR_INVALID, "seam distance: the mask and the distance plane must be 4-byte aligned");
    DenseWs* ws = nullptr;
    const int rc = rectify_dense_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    const int rm = ensure_plane(c, &ws->d_seam, (size_t)rows * (size_t)cols, "seam distance: no memory for the row pass's plane");
    if (rm != RSDSFM_OK) return rm;
    return seam_distance_launch(c, d_mask, rows, cols, feather ? feather : kFeatherDefault, ws->d_seam, d_dist_out);
}

int rsdsfm_seam_blend_layer_dev(rsdsfm_ctx* ctx, const uint8_t* d_layer_image, const uint8_t* d_layer_mask, int32_t channels, int32_t rows, int32_t cols,
                                const uint8_t* d_dist, const rsdsfm_stabilize_blend_params* params_or_null, int32_t source_id, uint8_t* d_image_inout,
                                uint8_t* d_mask_inout, uint8_t* d_source_inout, uint64_t* d_sums_out, int64_t* d_counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "seam blend: rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "seam blend: channels must be 1 or 3");
    if (!d_layer_image || !d_layer_mask || !d_dist || !d_image_inout || !d_mask_inout || !d_source_inout || !d_sums_out)
        return fail(c, RSDSFM_ERR_INVALID, "seam blend: null device pointer (the source plane and the sums record are required)");
    const uint8_t* in[3] = {d_layer_image, d_layer_mask, d_dist};
    const uint8_t* io[3] = {d_image_inout, d_mask_inout, d_source_inout};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (in[i] == io[j] || (i < j && io[i] == io[j])) return fail(c, RSDSFM_ERR_INVALID, "seam blend: the layer, the distance plane and the in-out planes may not alias");
    if (((uintptr_t)d_layer_image | (uintptr_t)d_layer_mask | (uintptr_t)d_dist | (uintptr_t)d_image_inout | (uintptr_t)d_mask_inout | (uintptr_t)d_source_inout) & 3u)
        return fail(c, RSDSFM_ERR_INVALID, "seam blend: every plane must be 4-byte aligned");
    if (((uintptr_t)d_sums_out | (uintptr_t)d_counts_or_null) & 7u) return fail(c, RSDSFM_ERR_INVALID, "seam blend: the sums and the counters must be 8-byte aligned");
    if (source_id < 2 || source_id > 255) return fail(c, RSDSFM_ERR_INVALID, "seam blend: source_id must be in [2, 255] (1 is the own frame, 0 nobody)");
    rsdsfm_stabilize_blend_params bp;
    if (!blend_params_resolve(params_or_null, &bp)) return fail(c, RSDSFM_ERR_INVALID, kBlendParamsMessage);
    return seam_blend_launch(c, d_layer_image, d_layer_mask, channels, rows, cols, d_dist, bp.feather, bp.min_overlap, bp.gain_mode, source_id, d_image_inout, d_mask_inout,
                             d_source_inout, reinterpret_cast<unsigned long long*>(d_sums_out), d_counts_or_null);
}

int rsdsfm_stabilize_video_blended_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
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
                                       int32_t window_out[4], int64_t* crop_counts_or_null, const rsdsfm_stabilize_blend_params* blend_params_or_null,
                                       uint8_t* const* d_blend_images, uint8_t* const* d_blend_masks, uint8_t* const* d_blend_sources, uint32_t* gains_or_null,
                                       int64_t* blend_counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (nframes < 2) return fail(c, RSDSFM_ERR_INVALID, "stabilise video: nframes must be >= 2");
    const int np = stabilize_rendered_frames(stabilize_params_or_null, nframes);  // rendered frames: the pairs' first frames, and the last frame when asked for
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "blend: rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "blend: channels must be 1 or 3");
    rsdsfm_stabilize_blend_params bp;
    if (!blend_params_resolve(blend_params_or_null, &bp)) return fail(c, RSDSFM_ERR_INVALID, kBlendParamsMessage);
    if (!all_set(d_blend_images, np) || !all_set(d_blend_masks, np) || !all_set(d_blend_sources, np))
        return fail(c, RSDSFM_ERR_INVALID, "blend: d_blend_images, d_blend_masks and d_blend_sources are required");
    for (int p = 0; p < np; ++p) {
        if (((uintptr_t)d_blend_images[p] | (uintptr_t)d_blend_masks[p] | (uintptr_t)d_blend_sources[p]) & 3u)
            return fail(c, RSDSFM_ERR_INVALID, "blend: blend images, masks and source planes must be 4-byte aligned");
        if (d_blend_sources[p] == d_blend_masks[p] || d_blend_images[p] == d_blend_masks[p] || d_blend_images[p] == d_blend_sources[p])
            return fail(c, RSDSFM_ERR_INVALID, "blend: a frame's blend planes must be distinct");
    }
    // the cropped clip: the public entry point itself, so that it runs the code it runs alone (and refuses what it refuses)
    int rc = rsdsfm_stabilize_video_cropped_dev(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds, d_flows,
                                                d_depth_maps, d_R, d_t, results, check_params_or_null, d_masks_or_null, link_params_or_null, records, scales, A, c_,
                                                broken_or_null, fuse_params_or_null, d_fused_maps_or_null, stabilize_params_or_null, mode, q5_mode, iterations, A_s, c_s, M,
                                                m, d_stab_images, d_masks_out, valid_or_null, fill_params_or_null, d_sources_or_null, counts_or_null, crop_params_or_null,
                                                window_in_or_null, d_crop_images, d_crop_masks, d_crop_sources_or_null, window_out, crop_counts_or_null);
    if (rc != RSDSFM_OK) return rc;
    const int radius = fill_params_or_null ? fill_params_or_null->radius : kBlendFillRadiusDefault;  // 0 .. 16: the inner call checked it
    const bool occ = visible_asked(fill_params_or_null);  // every layer is rendered through the occlusion test (the inner call checked the words)
    const int offs = 2 * radius;
    const size_t plane = (size_t)rows * (size_t)cols;
    const bool have = window_out[2] >= 1, host = gains_or_null || blend_counts_or_null;
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    rc = ensure_plane(c, &ws->d_layer, blend_layer_bytes(rows, cols), "blend: no memory for the distance plane and the layer");
    if (rc != RSDSFM_OK) return rc;
    const BlendLayer l = blend_layer(ws->d_layer, rows, cols);  // l.record: the record of a call without host arrays, every layer's in turn
    // with a host array: per frame [sums: offs x 8][own: 1][(filled, blended): offs x 2], 8-byte words
    const size_t per = (size_t)offs * 8 + 1 + (size_t)offs * 2;
    uint64_t* d_rec = nullptr;
    if (host && have) {
        RSDSFM_HIP_CHECK(c, hipMalloc(reinterpret_cast<void**>(&d_rec), sizeof(uint64_t) * (size_t)np * per));
        const hipError_t e = hipMemsetAsync(d_rec, 0, sizeof(uint64_t) * (size_t)np * per, c->stream);
        if (e != hipSuccess) {
            (void)hipFree(d_rec);
            RSDSFM_HIP_CHECK(c, e);
        }
    }
    int32_t frames[2 * kBlendFillRadiusMax], ids[2 * kBlendFillRadiusMax], listed = 0;
    double nM[9 * 2 * kBlendFillRadiusMax], nm[3 * 2 * kBlendFillRadiusMax];
    for (int p = 0; p < np && rc == RSDSFM_OK; ++p) {
        if (hipMemsetAsync(d_blend_images[p], 0, plane * (size_t)channels, c->stream) != hipSuccess || hipMemsetAsync(d_blend_masks[p], 0, plane, c->stream) != hipSuccess ||
            hipMemsetAsync(d_blend_sources[p], 0, plane, c->stream) != hipSuccess)
            rc = fail(c, RSDSFM_ERR_HIP, "blend: zeroing the blend planes failed");
        if (!have || rc != RSDSFM_OK) continue;
        uint64_t* rec = d_rec ? d_rec + (size_t)p * per : nullptr;
        const double* map = d_fused_maps_or_null ? d_fused_maps_or_null[p] : d_depth_maps[p];
        rc = rsdsfm_stabilize_window_frame_dev(ctx, d_frames[p], channels, map, d_R[p], d_t[p], fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, M + 9 * (size_t)p,
                                               m + 3 * (size_t)p, 1, window_out, d_blend_images[p], d_blend_masks[p], d_blend_sources[p],
                                               rec ? reinterpret_cast<int64_t*>(rec + (size_t)offs * 8) : nullptr);
        if (rc == RSDSFM_OK) rc = rsdsfm_seam_distance_dev(ctx, d_blend_masks[p], rows, cols, bp.feather, l.dist);
        listed = 0;
        if (rc == RSDSFM_OK && radius > 0 && rsdsfm_neighbour_poses(A, c_, A_s, c_s, scales, np, p, radius, frames, ids, nM, nm, &listed) != RSDSFM_OK)
            rc = fail(c, RSDSFM_ERR_INVALID, "blend: a neighbour's scale is not finite and positive");
        for (int k = 0; k < listed && rc == RSDSFM_OK; ++k) {
            const int n = frames[k], slot = ids[k] - 2;
            if (hipMemsetAsync(l.image, 0, plane * (size_t)channels, c->stream) != hipSuccess || hipMemsetAsync(l.mask, 0, plane, c->stream) != hipSuccess) {
                rc = fail(c, RSDSFM_ERR_HIP, "blend: zeroing the layer failed");
                break;
            }
            const double* nmap = d_fused_maps_or_null ? d_fused_maps_or_null[n] : d_depth_maps[n];
            rc = render_candidate(ctx, occ, occ ? fill_params_or_null->occlusion_tol_q16 : 0, d_frames[n], channels, nmap, d_R[n], d_t[n], fx, fy, cx, cy, rows, cols, mode,
                                  q5_mode, iterations, nM + 9 * (size_t)k, nm + 3 * (size_t)k, ids[k], window_out, l.image, l.mask, nullptr, nullptr);
            if (rc == RSDSFM_OK)
                rc = rsdsfm_seam_blend_layer_dev(ctx, l.image, l.mask, channels, rows, cols, l.dist, &bp, ids[k], d_blend_images[p], d_blend_masks[p], d_blend_sources[p],
                                                 rec ? rec + (size_t)slot * 8 : l.record,
                                                 rec ? reinterpret_cast<int64_t*>(rec + (size_t)offs * 8 + 1 + (size_t)slot * 2) : nullptr);
        }
    }
    std::vector<uint64_t> got;
    if (d_rec) {
        got.resize((size_t)np * per);
        hipError_t e = rc == RSDSFM_OK ? hipMemcpyAsync(got.data(), d_rec, sizeof(uint64_t) * got.size(), hipMemcpyDeviceToHost, c->stream) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        (void)hipFree(d_rec);
        if (rc == RSDSFM_OK) RSDSFM_HIP_CHECK(c, e);
    } else if (host && rc == RSDSFM_OK) {
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    }
    if (rc != RSDSFM_OK || !host) return rc;
    for (int p = 0; p < np; ++p) {
        const uint64_t* rec = have ? got.data() + (size_t)p * per : nullptr;
        if (gains_or_null)
            for (int k = 0; k < offs; ++k) {
                uint32_t* g = gains_or_null + ((size_t)p * offs + k) * 3;
                g[0] = g[1] = g[2] = kGainOne;
                if (rec) (void)rsdsfm_seam_gains(rec + (size_t)k * 8, channels, bp.min_overlap, bp.gain_mode, g);
            }
        if (blend_counts_or_null) {
            int64_t* row = blend_counts_or_null + (size_t)p * (2 + 2 * (size_t)offs);
            int64_t own = rec ? (int64_t)rec[(size_t)offs * 8] : 0, filled = 0, blended = 0;
            for (int k = 0; k < offs; ++k) {
                filled += (row[2 + 2 * k] = rec ? (int64_t)rec[(size_t)offs * 8 + 1 + 2 * k] : 0);
                blended += (row[3 + 2 * k] = rec ? (int64_t)rec[(size_t)offs * 8 + 2 + 2 * k] : 0);
            }
            row[0] = (int64_t)plane - own - filled;
            row[1] = own - blended;
        }
    }
    return RSDSFM_OK;
}

}  // extern "C"
