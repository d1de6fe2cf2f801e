// stabilize.hpp -- the stabiliser (include/rsdsfm_stabilize.h): what stabilize_kernels.hip and stabilize_host.hip share.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "rectify_dense.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

// host arithmetic the path smoother (stabilize_host.hip), the neighbours' poses (stabilize_fill_host.hip) and the retimer (retime_host.hip)
// share, operation by operation tests/stabilize_spec_numpy.py's

// a b for row-major 3 x 3, every entry (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j; ta: a transposed
inline void mat3(const double* a, bool ta, const double* b, double* out) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double a0 = ta ? a[i] : a[3 * i], a1 = ta ? a[3 + i] : a[3 * i + 1], a2 = ta ? a[6 + i] : a[3 * i + 2];
            out[3 * i + j] = (a0 * b[j] + a1 * b[3 + j]) + a2 * b[6 + j];
        }
}

// the rotation vector of R (tests/stabilize_spec_numpy.py: so3_log)
inline void so3_log(const double* R, double* l) {
    const double a[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double s = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    const double cc = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double theta = std::atan2(s, cc);
    const double f = s < 1e-8 ? 1.0 : theta / s;
    for (int i = 0; i < 3; ++i) l[i] = s < 1e-8 ? a[i] : a[i] * f;
}

// frame n seen from the camera (As, cs): M = As^T An, m = As^T (cn - cs) / S (tests/stabilize_fill_spec_numpy.py: neighbour_pose)
inline void pose_from(const double* As, const double* cs, const double* An, const double* cn, double S, double* M9, double* m3) {
    const double dc[3] = {cn[0] - cs[0], cn[1] - cs[1], cn[2] - cs[2]};
    for (int i = 0; i < 3; ++i) {  // row i of As^T: the spec's _mat3 and _matvec
        const double a0 = As[i], a1 = As[3 + i], a2 = As[6 + i];
        for (int j = 0; j < 3; ++j) M9[3 * i + j] = (a0 * An[j] + a1 * An[3 + j]) + a2 * An[6 + j];
        m3[i] = ((a0 * dc[0] + a1 * dc[1]) + a2 * dc[2]) / S;
    }
}

// the virtual pose of one frame, a kernel argument: X_virtual = M X_first_scanline + m (M row-major)
struct StabPose {
    double M[9];
    double m[3];
};

// the launches of one frame on c->stream (arguments checked by the caller; iterations 1 .. 16): the dense rectifier's stage A, the
// stabiliser's map kernel, the dense rectifier's stage C and, when d_valid is set, the count of d_mask (then not NULL)
int stabilize_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img, int channels, const double* d_depth_cm, const double* d_R, const double* d_t, double fx,
                     double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp, unsigned char* d_out,
                     unsigned char* d_mask, double* d_filled_cm, int64_t* d_valid);

}  // namespace rsdsfm
