// erase_host.hip -- C ABI of the mover removal (include/rsdsfm_erase.h; tests/erase_spec_numpy.py is the definition, erase_kernels.hip the
// kernels): the matte call, the composite call, the frame call, which CALLS the public plate, matte and composite entry points one after another
// on planes of the context's dense workspace, and the clip call, which calls the frame call per frame.
#include "clip_stage_host.hpp"
#include "erase.hpp"
#include "plate.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {
namespace {

// the resolved parameters: the plate's fields as the plate resolves them, and literal o, g, T
struct EraseResolved {
    rsdsfm_plate_params plate;
    int open, grow, feather, include_undecided;
};

const char* const kEraseParamsMessage =
    "rsdsfm_erase_params: open in [1, 3], 0 (the default, 2) or -1 (none), grow in [1, 8], 0 (the default, 2) or -1 (none), feather in [1, 16] or 0 (the default, 4), "
    "include_undecided 0 or 1, reserved words 0, struct_bytes 0 or sizeof (use rsdsfm_erase_params_init), and the plate's fields as rsdsfm_plate_params has them";

// NULL: the defaults; false: refused
bool erase_params_resolve(const rsdsfm_erase_params* in, EraseResolved* out) {
    if (!in) {
        out->open = kEraseOpenDefault, out->grow = kEraseGrowDefault, out->feather = kEraseFeatherDefault, out->include_undecided = 0;
        return plate_params_resolve(nullptr, &out->plate);
    }
    if (!struct_bytes_ok(in->struct_bytes, sizeof(rsdsfm_erase_params))) return false;
    for (int i = 0; i < 5; ++i)
        if (in->reserved[i] != 0) return false;
    const rsdsfm_plate_params pp{in->radius, in->threshold, in->min_votes, in->gain_mode, in->occlusion, in->occlusion_tol_q16, 0, 0, in->min_overlap, {0, 0, 0, 0}};
    if (!plate_params_resolve(&pp, &out->plate)) return false;
    out->plate.struct_bytes = (int32_t)sizeof(rsdsfm_plate_params);
    out->open = in->open == 0 ? kEraseOpenDefault : in->open == -1 ? 0 : in->open;
    out->grow = in->grow == 0 ? kEraseGrowDefault : in->grow == -1 ? 0 : in->grow;
    out->feather = in->feather == 0 ? kEraseFeatherDefault : in->feather;
    out->include_undecided = in->include_undecided;
    return in->open >= -1 && in->open <= kEraseOpenMax && in->grow >= -1 && in->grow <= kEraseGrowMax && in->feather >= 0 && in->feather <= kEraseFeatherMax &&
           (in->include_undecided == 0 || in->include_undecided == 1);
}

}  // namespace
}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_erase_params_init(rsdsfm_erase_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    rsdsfm_plate_params pp;
    (void)plate_params_resolve(nullptr, &pp);  // the plate's defaults
    *params = rsdsfm_erase_params{pp.radius, pp.threshold, pp.min_votes, pp.gain_mode, pp.occlusion, pp.occlusion_tol_q16, (int32_t)sizeof(rsdsfm_erase_params), kEraseOpenDefault,
                                  pp.min_overlap, kEraseGrowDefault, kEraseFeatherDefault, 0, {0, 0, 0, 0, 0}};
    return RSDSFM_OK;
}

int rsdsfm_mover_matte_launches(int32_t rows, int32_t cols) { return frame_size_ok(rows, cols) ? 3 : RSDSFM_ERR_INVALID; }

int rsdsfm_erase_composite_launches(void) { return 1; }

int rsdsfm_erase_launches(int32_t rows, int32_t cols, int32_t nsrc) {
    const int plate = rsdsfm_plate_launches(rows, cols, nsrc);
    if (plate < 0) return plate;
    return plate + rsdsfm_mover_matte_launches(rows, cols) + rsdsfm_erase_composite_launches();
}

int rsdsfm_mover_matte_dev(rsdsfm_ctx* ctx, const uint8_t* d_flag, int32_t rows, int32_t cols, int32_t open, int32_t grow, int32_t feather,
                           int32_t include_undecided, uint8_t* d_matte_out) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "mover matte: rows and cols must be in [2, 16384]");
    if (open < 0 || open > kEraseOpenMax || grow < 0 || grow > kEraseGrowMax || feather < 1 || feather > kEraseFeatherMax || (include_undecided != 0 && include_undecided != 1))
        return fail(c, RSDSFM_ERR_INVALID, "mover matte: open must be in [0, 3], grow in [0, 8], feather in [1, 16] and include_undecided 0 or 1");
    if (!d_flag || !d_matte_out || d_flag == d_matte_out) return fail(c, RSDSFM_ERR_INVALID, "mover matte: null or aliased device pointer");
    if (((uintptr_t)d_flag | (uintptr_t)d_matte_out) & 3u) return fail(c, RSDSFM_ERR_INVALID, "mover matte: the flag and the matte plane must be 4-byte aligned");
    DenseWs* ws = nullptr;
    int rc = rectify_dense_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    rc = ensure_plane(c, &ws->d_matte, matte_ws_bytes(rows, cols), "mover matte: no memory for the two intermediate planes");
    if (rc != RSDSFM_OK) return rc;
    return mover_matte_launch(c, d_flag, rows, cols, open, grow, feather, include_undecided, ws->d_matte, ws->d_matte + blend_plane_bytes(rows, cols), d_matte_out);
}

int rsdsfm_erase_composite_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* d_plate_image, const uint8_t* d_plate_mask,
                               const uint8_t* d_matte, int32_t channels, int32_t rows, int32_t cols, int32_t feather, uint8_t* d_image_out, uint8_t* d_mask_out,
                               int64_t* d_counts5_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "erase composite: rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "erase composite: channels must be 1 or 3");
    if (feather < 1 || feather > kEraseFeatherMax) return fail(c, RSDSFM_ERR_INVALID, "erase composite: feather must be in [1, 16]");
    const void* in[5] = {d_ref_image, d_ref_mask, d_plate_image, d_plate_mask, d_matte};
    const void* out[3] = {d_image_out, d_mask_out, d_counts5_or_null};
    for (int i = 0; i < 5; ++i)
        if (!in[i] || ((uintptr_t)in[i] & 3u)) return fail(c, RSDSFM_ERR_INVALID, "erase composite: null or misaligned input plane (4 bytes)");
    if (!d_image_out || !d_mask_out || (((uintptr_t)d_image_out | (uintptr_t)d_mask_out) & 3u))
        return fail(c, RSDSFM_ERR_INVALID, "erase composite: null or misaligned output plane (4 bytes)");
    if ((uintptr_t)d_counts5_or_null & 7u) return fail(c, RSDSFM_ERR_INVALID, "erase composite: the counters must be 8-byte aligned");
    if (d_ref_image == d_ref_mask || d_plate_image == d_plate_mask || d_matte == d_ref_image || d_matte == d_ref_mask || d_matte == d_plate_image || d_matte == d_plate_mask ||
        d_ref_image == d_plate_mask || d_plate_image == d_ref_mask)
        return fail(c, RSDSFM_ERR_INVALID, "erase composite: an image, a mask and the matte must be distinct planes");
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 5 && out[i]; ++j)
            if (out[i] == in[j]) return fail(c, RSDSFM_ERR_INVALID, "erase composite: an output may not be an input");
        for (int j = i + 1; j < 3; ++j)
            if (out[i] && out[i] == out[j]) return fail(c, RSDSFM_ERR_INVALID, "erase composite: the outputs must be distinct");
    }
    return erase_composite_launch(c, d_ref_image, d_ref_mask, d_plate_image, d_plate_mask, d_matte, channels, rows, cols, feather, d_image_out, d_mask_out, d_counts5_or_null);
}

int rsdsfm_erase_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                           const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                           int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_erase_params* params_or_null,
                           const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_matte_or_null, uint8_t* d_moving_or_null,
                           int64_t* d_counts5_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc < 1 || nsrc > kPlateSourcesMax) return fail(c, RSDSFM_ERR_INVALID, "erase frame: nsrc must be in [1, 15]");
    EraseResolved ep;
    if (!erase_params_resolve(params_or_null, &ep)) return fail(c, RSDSFM_ERR_INVALID, kEraseParamsMessage);
    rc = output_planes_check(c, "erase", {d_image_out, d_mask_out, d_matte_or_null, d_moving_or_null}, d_counts5_or_null, true);
    if (rc != RSDSFM_OK) return rc;
    if (!d_images) return fail(c, RSDSFM_ERR_INVALID, "erase frame: null source array");
    for (int k = 0; k < nsrc; ++k)  // the plate call checks the sources against ITS outputs, which are the workspace's
        if (d_images[k] && (d_images[k] == d_image_out || d_images[k] == d_mask_out || d_images[k] == d_matte_or_null || d_images[k] == d_moving_or_null))
            return fail(c, RSDSFM_ERR_INVALID, "erase frame: a source image may not be an output");
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);  // a size change releases the planes below with the rest
    if (rc != RSDSFM_OK) return rc;
    rc = ensure_plane(c, &ws->d_erase, erase_ws_bytes(rows, cols), "erase frame: no memory for the plate, the flag and the matte");
    if (rc != RSDSFM_OK) return rc;
    const size_t P = blend_plane_bytes(rows, cols);
    uint8_t* pmask = ws->d_erase;
    uint8_t* flag = d_moving_or_null ? d_moving_or_null : ws->d_erase + P;
    uint8_t* matte = d_matte_or_null ? d_matte_or_null : ws->d_erase + 2 * P;
    uint8_t* pimage = ws->d_erase + 3 * P;
    // 1. the public entry points themselves, so that they run the code they run alone; the plate call refuses before it enqueues
    rc = rsdsfm_plate_frame_dev(ctx, d_images, channels, d_depths_colmajor, d_R_rows9, d_t_rows3, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, nsrc, M, m, &ep.plate,
                                window_or_null, pimage, pmask, nullptr, flag, nullptr);
    if (rc != RSDSFM_OK) return rc;
    // 2. the own frame through the window with id 1 on zeroed planes: the plate call's reference planes, where it left them
    const PlatePlanes r = plate_planes(ws->d_plate, rows, cols);
    // 3., 4.
    rc = rsdsfm_mover_matte_dev(ctx, flag, rows, cols, ep.open, ep.grow, ep.feather, ep.include_undecided, matte);
    if (rc != RSDSFM_OK) return rc;
    return rsdsfm_erase_composite_dev(ctx, r.rimage, r.rmask, pimage, pmask, matte, channels, rows, cols, ep.feather, d_image_out, d_mask_out, d_counts5_or_null);
}

int rsdsfm_erase_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                           double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                           const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                           const rsdsfm_erase_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks,
                           uint8_t* const* d_out_mattes_or_null, uint8_t* const* d_out_moving_or_null, int64_t* counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    ClipOutputs outs;
    outs.planes[0] = d_out_images;
    outs.planes[1] = d_out_masks;
    outs.planes[2] = d_out_mattes_or_null;
    outs.planes[3] = d_out_moving_or_null;
    const int rc = clip_arrays_check(c, "erase video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, outs,
                                     "its matte and flag planes when their arrays are passed");
    if (rc != RSDSFM_OK) return rc;
    EraseResolved ep;
    if (!erase_params_resolve(params_or_null, &ep)) return fail(c, RSDSFM_ERR_INVALID, kEraseParamsMessage);
    // the public entry point itself, so that it runs the code it runs alone
    return walk_clip(c, "erase video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, ep.plate.radius, outs, 5, counts_or_null,
                     [&](const ClipFrame& f) {
                         return rsdsfm_erase_frame_dev(ctx, f.img, channels, f.map, f.R, f.t, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, f.plan->nsrc, f.plan->M, f.plan->m,
                                                       params_or_null, window_or_null, f.out[0], f.out[1], f.out[2], f.out[3], f.d_counts);
                     });
}

}  // extern "C"
