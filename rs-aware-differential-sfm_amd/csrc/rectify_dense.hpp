// rectify_dense.hpp -- the dense global-shutter rectifier (include/rsdsfm_rectify_dense.h): what rectify_dense_kernels.hip,
// rectify_dense_host.hip and rectify_dense_video_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rsdsfm_internal.hpp"

namespace rsdsfm {

// The context's (and so every lane's) workspace, Ctx::rectify_dense: the pull-push pyramid from level 1 up (level 0 is the depth map itself,
// read in place) and the displacement plane of stage B.  Made on first use and again when the image size changes (rectify_dense_ws).
struct DenseWs {
    double* d_pyr = nullptr;  // levels 1 .. top, level after level, row-major
    float2* d_disp = nullptr; // rows x cols
    unsigned char* d_mask = nullptr;  // rows x cols: the stabiliser's mask when it counts without a caller's mask (made when first asked for)
    void* d_crop = nullptr;           // the crop window's key, plane pointers and summed-area table (stabilize_crop.hpp; made when first asked for)
    unsigned char* d_seam = nullptr;  // rows x cols: the seam distance's row pass (stabilize_blend.hpp; made when first asked for)
    unsigned char* d_layer = nullptr; // the blended clip's distance plane, layer mask and layer image, 5 planes (stabilize_blend.hpp; made when first asked for)
    void* d_inpaint = nullptr;        // the inpainting's pyramid of 8-byte cells and its validity word (stabilize_inpaint.hpp; made when first asked for)
    void* d_visible = nullptr;        // the occlusion test's planes: zv (rows x cols float) and zbuf (rows x cols uint32) behind it (stabilize_visible.hpp; made when first asked for)
    void* d_search = nullptr;         // the visible pre-image search's planes: kbuf (rows x cols uint64) and a zv behind it (stabilize_search.hpp; made when first asked for)
    unsigned char* d_layer2 = nullptr; // the retimer's second layer, mask and image, 4 planes (retime.hpp; made when first asked for)
    unsigned char* d_shutter = nullptr; // the synthetic shutter's sample mask and image and its cells, 12 planes (shutter.hpp; made when first asked for)
    unsigned char* d_denoise = nullptr; // the temporal denoise's reference mask, source plane and image and its cells, 13 planes (denoise.hpp; made when first asked for)
    unsigned char* d_superres = nullptr; // the super-resolution's own planes, layer planes, cells and record on the FINE grid, 23 planes (superres.hpp; made when first asked for)
    int superres_scale = 0;              // the scale d_superres was made for
    unsigned char* d_plate = nullptr;    // the clean plate's reference planes, records and stack of layers (plate.hpp; made when first asked for)
    int plate_layers = 0;                // the layers d_plate holds
    unsigned char* d_matte = nullptr;    // the mover matte's two intermediate planes (erase.hpp; made when first asked for)
    unsigned char* d_erase = nullptr;    // the mover removal's plate mask, flag, matte and plate image, 6 planes (erase.hpp; made when first asked for)
    unsigned long long* d_deblur = nullptr; // the sharpness transfer's one record, 4 words; its planes are d_denoise's and d_layer's (deblur.hpp; made when first asked for)
    unsigned long long* d_deblur_bands = nullptr; // its band records, 64 x 4 words whatever the size (deblur.hpp; made when a frame call with band_rows first asks for it)
    unsigned char* d_denoise_spatial = nullptr; // the spatial top-up's frame call: the temporal stage's weight and image, 4 planes (denoise.hpp; made when first asked for)
    unsigned char* d_noise = nullptr; // the noise level's histogram (1024 uint32) and a record (4 uint64) for the auto frame call (noise.hpp; made when first asked for)
    unsigned char* d_noise_curve = nullptr; // the noise curve's histogram (8 x 1024 uint32) and a curve (36 uint64) for the curve frame call (noise_curve.hpp; made when first asked for)
    unsigned char* d_noise_temporal = nullptr; // the temporal noise curve's frame call: the neighbours' records and the stack of their layers (noise_temporal.hpp; made when first asked for)
    size_t noise_temporal_bytes = 0;           // the bytes d_noise_temporal holds
    int rows = 0, cols = 0;
};

// geometry of the pyramid of a rows x cols map: level l (1 .. nl) has h[l - 1] x w[l - 1] cells at off[l - 1] doubles
constexpr int kDenseMaxLevels = 16;  // 16384 -> 8192 = 2^13 -> ... -> 1: 14 levels
struct DensePlan {
    int nl = 0, small = 0;  // small: index of the first level of the single-workgroup launch (everything from it up fits its LDS)
    int h[kDenseMaxLevels], w[kDenseMaxLevels];
    size_t off[kDenseMaxLevels], total = 0;
};
DensePlan rectify_dense_plan(int rows, int cols);
int rectify_dense_launch_count(int rows, int cols);  // kernel launches of one frame

int rectify_dense_ws(Ctx* c, int rows, int cols, DenseWs** ws);  // rectify_dense_host.hip
void rectify_dense_release(Ctx* c);

// the launches of one frame on c->stream (arguments checked by the caller; iterations 1 .. 16)
int rectify_dense_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img, int channels, const double* d_depth_cm, const double* d_R, const double* d_t,
                         double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, unsigned char* d_out,
                         unsigned char* d_mask, double* d_filled_cm);
// its parts, for the stabiliser (stabilize_kernels.hip), which puts a map kernel of its own between them: stage A (*top: the 1 x 1 level,
// in the workspace) and stage C
int rectify_dense_launch_fill(Ctx* c, const DenseWs& ws, const double* d_depth_cm, int rows, int cols, const double** top);
int rectify_dense_launch_warp(Ctx* c, const DenseWs& ws, const unsigned char* d_img, int channels, const double* top, int rows, int cols, int iterations,
                              unsigned char* d_out, unsigned char* d_mask);
// the argument checks both entry points share (everything but the context and the sizes of the clip)
int rectify_dense_check(Ctx* c, int channels, int rows, int cols, int mode, int q5_mode, int iterations);

}  // namespace rsdsfm
