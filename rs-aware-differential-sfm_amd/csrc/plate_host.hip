// plate_host.hip -- C ABI of the clean plate (include/rsdsfm_plate.h; tests/plate_spec_numpy.py is the definition, plate_kernels.hip the
// kernel) and of its colour-consistent estimator (include/rsdsfm_plate_medoid.h; tests/plate_medoid_spec_numpy.py, plate_medoid_kernels.hip):
// the median call and the medoid call behind one argument check, the context's knob between them, the frame call, which CALLS the public
// render entry points, the record call and the estimator one after another on planes of the context's dense workspace, and the clip call,
// which calls the frame call per frame.
#include "clip_stage_host.hpp"
#include "plate.hpp"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"
#include "stabilize_blend.hpp"

namespace rsdsfm {
namespace {

rsdsfm_plate_params plate_defaults() {
    return rsdsfm_plate_params{RSDSFM_PLATE_RADIUS_DEFAULT, kPlateThresholdDefault, kPlateMinVotesDefault, 0, 0, 0, (int32_t)sizeof(rsdsfm_plate_params), 0, kMinOverlapDefault,
                               {0, 0, 0, 0}};
}

// the workspace's reference planes, records and a stack of at least `layers` layers, made when first asked for and again when more layers are asked for
int plate_ws(Ctx* c, int rows, int cols, int layers, DenseWs** ws) {
    int rc = rectify_dense_ws(c, rows, cols, ws);  // a size change releases them with the rest
    if (rc != RSDSFM_OK) return rc;
    DenseWs* w = *ws;
    if (w->d_plate && w->plate_layers < layers) {  // behind whatever the stream still runs on the smaller stack
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(w->d_plate);
        w->d_plate = nullptr;
        w->plate_layers = 0;
    }
    if (!w->d_plate) {
        rc = ensure_plane(c, &w->d_plate, plate_ws_bytes(rows, cols, layers), "plate: no memory for the reference planes and the stack of layers");
        if (rc != RSDSFM_OK) return rc;
        w->plate_layers = layers;
    }
    return RSDSFM_OK;
}

// the argument checks of rsdsfm_plate_median_dev and rsdsfm_plate_medoid_dev, which take the same arguments and refuse the same ones, and the
// kernel's argument with every default resolved
int plate_call_args(Ctx* c, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* const* d_layer_images, const uint8_t* const* d_layer_masks, int32_t nlayers,
                    int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null, int64_t min_overlap, int32_t gain_mode, int32_t threshold, int32_t min_votes,
                    uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_votes_or_null, uint8_t* d_moving_or_null, int64_t* d_counts4_or_null, PlateArgs* out) {
    if (!frame_size_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "plate: rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "plate: channels must be 1 or 3");
    if (nlayers < 0 || nlayers > kPlateLayersMax) return fail(c, RSDSFM_ERR_INVALID, "plate median: nlayers must be in [0, 14]");
    if (min_overlap < 0 || (gain_mode != 0 && gain_mode != 1) || threshold < 0 || threshold > kPlateThresholdMax || min_votes < 0 || min_votes > kPlateMinVotesMax)
        return fail(c, RSDSFM_ERR_INVALID,
                    "plate median: min_overlap must be >= 0, gain_mode 0 or 1, threshold in [1, 255] (0: the default, 24) and min_votes in [1, 15] (0: the default, 3)");
    int rc = output_planes_check(c, "plate", {d_image_out, d_mask_out, d_votes_or_null, d_moving_or_null}, d_counts4_or_null, true);
    if (rc != RSDSFM_OK) return rc;
    if (!d_ref_image || !d_ref_mask || d_ref_image == d_ref_mask) return fail(c, RSDSFM_ERR_INVALID, "plate median: the reference needs its image and its mask");
    if (nlayers > 0 && (!d_layer_images || !d_layer_masks)) return fail(c, RSDSFM_ERR_INVALID, "plate median: the layers need their arrays of images and masks");
    if (((uintptr_t)d_ref_image | (uintptr_t)d_ref_mask) & 3u) return fail(c, RSDSFM_ERR_INVALID, "plate: every plane must be 4-byte aligned");
    if ((uintptr_t)d_sums8_or_null & 7u) return fail(c, RSDSFM_ERR_INVALID, "plate median: the records must be 8-byte aligned");
    const void* in[3 + 2 * kPlateLayersMax] = {d_ref_image, d_ref_mask, d_sums8_or_null};
    int nin = 3;
    for (int j = 0; j < nlayers; ++j) {
        const uint8_t *li = d_layer_images[j], *lm = d_layer_masks[j];
        if (!li || !lm) return fail(c, RSDSFM_ERR_INVALID, "plate median: every layer needs its image and its mask");
        if (((uintptr_t)li | (uintptr_t)lm) & 3u) return fail(c, RSDSFM_ERR_INVALID, "plate: every plane must be 4-byte aligned");
        if (li == lm || li == d_ref_image || li == d_ref_mask || lm == d_ref_image || lm == d_ref_mask)
            return fail(c, RSDSFM_ERR_INVALID, "plate median: the reference's and a layer's planes must be distinct");
        in[nin++] = li;
        in[nin++] = lm;
    }
    const void* io[5] = {d_image_out, d_mask_out, d_votes_or_null, d_moving_or_null, d_counts4_or_null};
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < nin && io[i]; ++j)
            if (in[j] == io[i]) return fail(c, RSDSFM_ERR_INVALID, "plate median: an output may not be an input or the records");
    PlateArgs& args = *out;
    args = PlateArgs{};
    args.ref = d_ref_image;
    args.rmask = d_ref_mask;
    for (int j = 0; j < nlayers; ++j) {
        args.layer[j] = d_layer_images[j];
        args.lmask[j] = d_layer_masks[j];
    }
    args.sums = nlayers > 0 ? reinterpret_cast<const unsigned long long*>(d_sums8_or_null) : nullptr;
    args.out = d_image_out;
    args.mask_out = d_mask_out;
    args.votes = d_votes_or_null;
    args.moving = d_moving_or_null;
    args.counts = reinterpret_cast<unsigned long long*>(d_counts4_or_null);
    args.min_overlap = min_overlap ? min_overlap : kMinOverlapDefault;
    args.rows = rows;
    args.cols = cols;
    args.nlayers = nlayers;
    args.gain_mode = gain_mode;
    args.threshold = (unsigned)(threshold ? threshold : kPlateThresholdDefault);
    args.min_votes = (unsigned)(min_votes ? min_votes : kPlateMinVotesDefault);
    return RSDSFM_OK;
}

static_assert(kPlateSourcesMax == kClipSourcesMax, "a frame's sources are a ClipPlan's");

}  // namespace

// the params with every 0 of radius, threshold, min_votes and min_overlap replaced by its default, or the defaults for NULL; false: refused
bool plate_params_resolve(const rsdsfm_plate_params* in, rsdsfm_plate_params* out) {
    *out = in ? *in : plate_defaults();
    if (!struct_bytes_ok(out->struct_bytes, sizeof(rsdsfm_plate_params))) return false;
    if (out->radius == 0) out->radius = RSDSFM_PLATE_RADIUS_DEFAULT;
    if (out->threshold == 0) out->threshold = kPlateThresholdDefault;
    if (out->min_votes == 0) out->min_votes = kPlateMinVotesDefault;
    if (out->min_overlap == 0) out->min_overlap = kMinOverlapDefault;
    return out->radius >= 1 && out->radius <= kPlateRadiusMax && out->threshold >= 1 && out->threshold <= kPlateThresholdMax && out->min_votes >= 1 &&
           out->min_votes <= kPlateMinVotesMax && out->min_overlap >= 0 && (out->gain_mode == 0 || out->gain_mode == 1) &&
           occlusion_words_ok(out->occlusion, out->occlusion_tol_q16);
}

const char* const kPlateParamsMessage =
    "rsdsfm_plate_params: radius in [1, 7] or 0, threshold in [1, 255] or 0, min_votes in [1, 15] or 0, gain_mode 0 or 1, occlusion 0 or 1, occlusion_tol_q16 in [0, 65536], "
    "min_overlap >= 0, struct_bytes 0 or sizeof (use rsdsfm_plate_params_init)";

}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_plate_params_init(rsdsfm_plate_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = plate_defaults();
    return RSDSFM_OK;
}

int rsdsfm_plate_median_launches(void) { return 1; }

int rsdsfm_plate_launches(int32_t rows, int32_t cols, int32_t nsrc) {
    if (nsrc < 1 || nsrc > kPlateSourcesMax) return RSDSFM_ERR_INVALID;
    const int one = rsdsfm_stabilize_window_launches(rows, cols);
    if (one < 0) return one;
    return nsrc * one + (nsrc - 1) + rsdsfm_plate_median_launches();
}

int rsdsfm_plate_median_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* const* d_layer_images,
                            const uint8_t* const* d_layer_masks, int32_t nlayers, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                            int64_t min_overlap, int32_t gain_mode, int32_t threshold, int32_t min_votes, uint8_t* d_image_out, uint8_t* d_mask_out,
                            uint8_t* d_votes_or_null, uint8_t* d_moving_or_null, int64_t* d_counts4_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    PlateArgs args;
    const int rc = plate_call_args(c, d_ref_image, d_ref_mask, d_layer_images, d_layer_masks, nlayers, channels, rows, cols, d_sums8_or_null, min_overlap, gain_mode, threshold,
                                   min_votes, d_image_out, d_mask_out, d_votes_or_null, d_moving_or_null, d_counts4_or_null, &args);
    if (rc != RSDSFM_OK) return rc;
    return plate_median_launch(c, args, channels);
}

int rsdsfm_plate_medoid_launches(void) { return 1; }

int rsdsfm_plate_medoid_dev(rsdsfm_ctx* ctx, const uint8_t* d_ref_image, const uint8_t* d_ref_mask, const uint8_t* const* d_layer_images,
                            const uint8_t* const* d_layer_masks, int32_t nlayers, int32_t channels, int32_t rows, int32_t cols, const uint64_t* d_sums8_or_null,
                            int64_t min_overlap, int32_t gain_mode, int32_t threshold, int32_t min_votes, uint8_t* d_image_out, uint8_t* d_mask_out,
                            uint8_t* d_votes_or_null, uint8_t* d_moving_or_null, int64_t* d_counts4_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    PlateArgs args;
    const int rc = plate_call_args(c, d_ref_image, d_ref_mask, d_layer_images, d_layer_masks, nlayers, channels, rows, cols, d_sums8_or_null, min_overlap, gain_mode, threshold,
                                   min_votes, d_image_out, d_mask_out, d_votes_or_null, d_moving_or_null, d_counts4_or_null, &args);
    if (rc != RSDSFM_OK) return rc;
    return plate_medoid_launch(c, args, channels);
}

int rsdsfm_set_plate_estimator(rsdsfm_ctx* ctx, int32_t estimator) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    if (estimator != RSDSFM_PLATE_MEDIAN && estimator != RSDSFM_PLATE_MEDOID)
        return fail(c, RSDSFM_ERR_INVALID, "rsdsfm_set_plate_estimator: 0 (the per-channel median) or 1 (the L1 medoid)");
    c->plate_estimator = estimator;
    return RSDSFM_OK;
}

int rsdsfm_plate_frame_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_images, int32_t channels, const double* const* d_depths_colmajor,
                           const double* const* d_R_rows9, const double* const* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows, int32_t cols,
                           int mode, int q5_mode, int32_t iterations, int32_t nsrc, const double* M, const double* m, const rsdsfm_plate_params* params_or_null,
                           const int32_t* window_or_null, uint8_t* d_image_out, uint8_t* d_mask_out, uint8_t* d_votes_or_null, uint8_t* d_moving_or_null,
                           int64_t* d_counts4_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (nsrc < 1 || nsrc > kPlateSourcesMax) return fail(c, RSDSFM_ERR_INVALID, "plate frame: nsrc must be in [1, 15]");
    rsdsfm_plate_params pp;
    if (!plate_params_resolve(params_or_null, &pp)) return fail(c, RSDSFM_ERR_INVALID, kPlateParamsMessage);
    rc = frame_sources_check(c, "plate frame", d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, nsrc, {d_image_out, d_mask_out, d_votes_or_null, d_moving_or_null});
    if (rc == RSDSFM_OK) rc = frame_poses_check(c, "plate frame", M, m, nsrc);
    if (rc == RSDSFM_OK) rc = output_planes_check(c, "plate", {d_image_out, d_mask_out, d_votes_or_null, d_moving_or_null}, d_counts4_or_null, true);
    int32_t full[4];
    const int32_t* window = nullptr;
    if (rc == RSDSFM_OK) rc = frame_window(c, "plate frame", window_or_null, rows, cols, full, &window);
    if (rc != RSDSFM_OK) return rc;
    DenseWs* ws = nullptr;
    const int nl = nsrc - 1;
    rc = plate_ws(c, rows, cols, nl, &ws);
    if (rc != RSDSFM_OK) return rc;
    const RenderGeom g{channels, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations};
    const size_t P = blend_plane_bytes(rows, cols);
    const PlatePlanes r = plate_planes(ws->d_plate, rows, cols);
    rc = render_reference(ctx, "plate frame", source_view(d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, 0), g, M, m, window, r.rimage, r.rmask, r.rsource);
    if (rc != RSDSFM_OK) return rc;
    const uint8_t *limages[kPlateLayersMax], *lmasks[kPlateLayersMax];
    for (int k = 1; k < nsrc; ++k) {
        uint8_t* lmask = r.stack + 4 * P * (size_t)(k - 1);  // every neighbour its own layer: the median sees them all at once
        uint8_t* limage = lmask + P;
        limages[k - 1] = limage;
        lmasks[k - 1] = lmask;
        rc = neighbour_step(ctx, "plate frame: zeroing a layer failed", pp.occlusion == 1, pp.occlusion_tol_q16, source_view(d_images, d_depths_colmajor, d_R_rows9, d_t_rows3, k), g,
                            M + 9 * k, m + 3 * k, window, r.rimage, r.rsource, limage, lmask, r.records + 8 * (size_t)(k - 1));
        if (rc != RSDSFM_OK) return rc;
    }
    // the public entry point of the context's estimator (rsdsfm_set_plate_estimator): the one place where the two part
    const auto estimate = c->plate_estimator == RSDSFM_PLATE_MEDOID ? rsdsfm_plate_medoid_dev : rsdsfm_plate_median_dev;
    return estimate(ctx, r.rimage, r.rmask, nl ? limages : nullptr, nl ? lmasks : nullptr, nl, channels, rows, cols, nl ? r.records : nullptr, pp.min_overlap, pp.gain_mode,
                    pp.threshold, pp.min_votes, d_image_out, d_mask_out, d_votes_or_null, d_moving_or_null, d_counts4_or_null);
}

int rsdsfm_plate_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nsources, int32_t rows, int32_t cols, int32_t channels, double fx, double fy,
                           double cx, double cy, const double* const* d_depth_maps, const double* const* d_R, const double* const* d_t, const double* A,
                           const double* c_, const double* A_path, const double* c_path, const double* scales, int mode, int q5_mode, int32_t iterations,
                           const rsdsfm_plate_params* params_or_null, const int32_t* window_or_null, uint8_t* const* d_out_images, uint8_t* const* d_out_masks,
                           uint8_t* const* d_out_votes_or_null, uint8_t* const* d_out_moving_or_null, int64_t* counts_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    ClipOutputs outs;
    outs.planes[0] = d_out_images;
    outs.planes[1] = d_out_masks;
    outs.planes[2] = d_out_votes_or_null;
    outs.planes[3] = d_out_moving_or_null;
    const int rc = clip_arrays_check(c, "plate video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, outs,
                                     "its votes and flag planes when their arrays are passed");
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_plate_params pp;
    if (!plate_params_resolve(params_or_null, &pp)) return fail(c, RSDSFM_ERR_INVALID, kPlateParamsMessage);
    // the public entry point itself, so that it runs the code it runs alone
    return walk_clip(c, "plate video", d_frames, nsources, d_depth_maps, d_R, d_t, A, c_, A_path, c_path, scales, pp.radius, outs, 4, counts_or_null, [&](const ClipFrame& f) {
        return rsdsfm_plate_frame_dev(ctx, f.img, channels, f.map, f.R, f.t, fx, fy, cx, cy, rows, cols, mode, q5_mode, iterations, f.plan->nsrc, f.plan->M, f.plan->m,
                                      params_or_null, window_or_null, f.out[0], f.out[1], f.out[2], f.out[3], f.d_counts);
    });
}

}  // extern "C"
