// rectify_dense_host.hip -- rsdsfm_rectify_dense_frame_dev (include/rsdsfm_rectify_dense.h): the argument checks, the context's workspace
// (pyramid + displacement plane, Ctx::rectify_dense) and the single-frame entry point; the kernels and their launches are in
// rectify_dense_kernels.hip.
#include "../../include/rsdsfm_rectify_dense.h"
#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

static void dense_ws_free(DenseWs* w) {
    if (w->d_pyr) (void)hipFree(w->d_pyr);
    if (w->d_disp) (void)hipFree(w->d_disp);
    if (w->d_mask) (void)hipFree(w->d_mask);
    if (w->d_crop) (void)hipFree(w->d_crop);
    if (w->d_seam) (void)hipFree(w->d_seam);
    if (w->d_layer) (void)hipFree(w->d_layer);
    if (w->d_inpaint) (void)hipFree(w->d_inpaint);
    if (w->d_visible) (void)hipFree(w->d_visible);
    w->d_visible = nullptr;
    if (w->d_search) (void)hipFree(w->d_search);
    w->d_search = nullptr;
    if (w->d_layer2) (void)hipFree(w->d_layer2);
    w->d_layer2 = nullptr;
    if (w->d_shutter) (void)hipFree(w->d_shutter);
    w->d_shutter = nullptr;
    if (w->d_denoise) (void)hipFree(w->d_denoise);
    w->d_denoise = nullptr;
    if (w->d_superres) (void)hipFree(w->d_superres);
    w->d_superres = nullptr;
    w->superres_scale = 0;
    if (w->d_plate) (void)hipFree(w->d_plate);
    w->d_plate = nullptr;
    w->plate_layers = 0;
    if (w->d_matte) (void)hipFree(w->d_matte);
    w->d_matte = nullptr;
    if (w->d_erase) (void)hipFree(w->d_erase);
    w->d_erase = nullptr;
    if (w->d_deblur) (void)hipFree(w->d_deblur);
    w->d_deblur = nullptr;
    if (w->d_deblur_bands) (void)hipFree(w->d_deblur_bands);
    w->d_deblur_bands = nullptr;
    if (w->d_denoise_spatial) (void)hipFree(w->d_denoise_spatial);
    w->d_denoise_spatial = nullptr;
    if (w->d_noise) (void)hipFree(w->d_noise);
    w->d_noise = nullptr;
    if (w->d_noise_curve) (void)hipFree(w->d_noise_curve);
    w->d_noise_curve = nullptr;
    if (w->d_noise_temporal) (void)hipFree(w->d_noise_temporal);
    w->d_noise_temporal = nullptr;
    w->noise_temporal_bytes = 0;
    w->d_pyr = nullptr;
    w->d_disp = nullptr;
    w->d_mask = nullptr;
    w->d_crop = nullptr;
    w->d_seam = nullptr;
    w->d_layer = nullptr;
    w->d_inpaint = nullptr;
    w->rows = w->cols = 0;
}

// the workspace for rows x cols images: made on first use, made again when the size changes (behind whatever the stream still runs on the old one)
int rectify_dense_ws(Ctx* c, int rows, int cols, DenseWs** out) {
    DenseWs* w = static_cast<DenseWs*>(c->rectify_dense);
    if (!w) c->rectify_dense = w = new DenseWs();
    if (w->rows != rows || w->cols != cols) {
        if (w->d_pyr) RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        dense_ws_free(w);
        const DensePlan p = rectify_dense_plan(rows, cols);
        RSDSFM_HIP_CHECK(c, hipMalloc(reinterpret_cast<void**>(&w->d_pyr), sizeof(double) * p.total));
        if (hipMalloc(reinterpret_cast<void**>(&w->d_disp), sizeof(float2) * (size_t)rows * (size_t)cols) != hipSuccess) {
            dense_ws_free(w);
            return fail(c, RSDSFM_ERR_HIP, "dense rectifier: no memory for the displacement plane");
        }
        w->rows = rows, w->cols = cols;
    }
    *out = w;
    return RSDSFM_OK;
}

void rectify_dense_release(Ctx* c) {
    DenseWs* w = static_cast<DenseWs*>(c->rectify_dense);
    if (!w) return;
    dense_ws_free(w);
    delete w;
    c->rectify_dense = nullptr;
}

int rectify_dense_check(Ctx* c, int channels, int rows, int cols, int mode, int q5_mode, int iterations) {
    if (rows < 2 || cols < 2 || rows > 16384 || cols > 16384) return fail(c, RSDSFM_ERR_INVALID, "dense rectifier: rows and cols must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "dense rectifier: channels must be 1 or 3");
    if (mode != RSDSFM_BACKPROJECT_RS && mode != RSDSFM_BACKPROJECT_GS) return fail(c, RSDSFM_ERR_INVALID, "unknown back-projection mode");
    if (q5_mode != RSDSFM_Q5_COMPAT && q5_mode != RSDSFM_Q5_FIXED) return fail(c, RSDSFM_ERR_INVALID, "unknown q5_mode");
    if (iterations < 0 || iterations > 16) return fail(c, RSDSFM_ERR_INVALID, "dense rectifier: iterations must be 1..16, or 0 for the default");
    return RSDSFM_OK;
}

}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_rectify_dense_launches(int32_t rows, int32_t cols) {
    if (rows < 2 || cols < 2 || rows > 16384 || cols > 16384) return RSDSFM_ERR_INVALID;
    return rectify_dense_launch_count(rows, cols);
}

int rsdsfm_rectify_dense_frame_dev(rsdsfm_ctx* ctx, const uint8_t* d_image, int32_t channels, const double* d_depth_map_colmajor,
                                   const double* d_R_rows9, const double* d_t_rows3, double fx, double fy, double cx, double cy, int32_t rows,
                                   int32_t cols, int mode, int q5_mode, int32_t iterations, uint8_t* d_dense_image, uint8_t* d_mask_or_null,
                                   double* d_filled_depth_or_null, float* d_disp_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = rectify_dense_check(c, channels, rows, cols, mode, q5_mode, iterations);
    if (rc != RSDSFM_OK) return rc;
    if (!d_image || !d_depth_map_colmajor || !d_R_rows9 || !d_t_rows3 || !d_dense_image || d_dense_image == d_image)
        return fail(c, RSDSFM_ERR_INVALID, "null or aliased device pointer");
    if (((uintptr_t)d_image | (uintptr_t)d_dense_image | (uintptr_t)d_mask_or_null) & 3u)
        return fail(c, RSDSFM_ERR_INVALID, "dense rectifier: images and mask must be 4-byte aligned");
    DenseWs* ws = nullptr;
    rc = rectify_dense_ws(c, rows, cols, &ws);
    if (rc != RSDSFM_OK) return rc;
    rc = rectify_dense_launch(c, *ws, d_image, channels, d_depth_map_colmajor, d_R_rows9, d_t_rows3, fx, fy, cx, cy, rows, cols, mode, q5_mode,
                              iterations ? iterations : 3, d_dense_image, d_mask_or_null, d_filled_depth_or_null);
    if (rc != RSDSFM_OK) return rc;
    if (d_disp_or_null)  // the caller's float pairs need not be 8-byte aligned: the kernels keep the plane of the workspace
        RSDSFM_HIP_CHECK(c, hipMemcpyAsync(d_disp_or_null, ws->d_disp, sizeof(float2) * (size_t)rows * (size_t)cols, hipMemcpyDeviceToDevice, c->stream));
    return RSDSFM_OK;
}

}  // extern "C"
