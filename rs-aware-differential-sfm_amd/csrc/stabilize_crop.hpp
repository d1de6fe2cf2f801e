// stabilize_crop.hpp -- the stabiliser's crop and zoom (include/rsdsfm_stabilize_crop.h): what stabilize_crop_kernels.hip and
// stabilize_crop_host.hip share.
#pragma once

#include <stdint.h>

#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize.hpp"
#include "stabilize_fill.hpp"

namespace rsdsfm {

constexpr int kCropPlanesMax = 4096;

// the planes of one search, a kernel argument would be too large for 4096 pointers: the host copies them behind the table
// (DenseWs::d_crop: [key: 8 B][planes: kCropPlanesMax pointers][table: (rows + 1) x (cols + 1) uint32])
struct CropWs {
    unsigned long long* d_key;
    const unsigned char** d_planes;
    unsigned* d_table;
};
CropWs crop_ws_layout(void* d_crop);
size_t crop_ws_bytes(int rows, int cols);

// the three launches of one search on c->stream (arguments checked by the caller; the planes' pointers already in ws.d_planes): the key is
// zeroed first and holds the winner's key, 0 = no window, when the stream has run
int crop_window_launch(Ctx* c, const CropWs& ws, int nmasks, int rows, int cols, int64_t max_empty, int margin);

// the winner's key (tests/stabilize_crop_spec_numpy.py::window_key): h << 45 | (131071 - dist) << 28 | (16383 - r) << 14 | (16383 - c)
void crop_decode_key(unsigned long long key, int rows, int cols, int32_t window[4]);

// the launches of one frame through a window on c->stream (arguments checked by the caller; iterations 1 .. 16): the dense rectifier's
// stage A, the stabiliser's map kernel with vp, and the window-warp kernel in stage C's place; as stabilize_fill_launch otherwise
int stabilize_window_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img_n, int channels, const double* d_depth_cm, const double* d_R, const double* d_t,
                            double fx, double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp, int source_id,
                            const int32_t window[4], unsigned char* d_out, unsigned char* d_mask, unsigned char* d_source, int64_t* d_filled);

}  // namespace rsdsfm
