// last_frame_host.hip -- C ABI of the clip's last frame (include/rsdsfm_last_frame.h; tests/last_frame_spec_numpy.py is the definition,
// last_frame_kernels.hip the kernels): the advance of a pair's depth map onto its second frame, the motion of that frame in the pose
// table's form (host arithmetic), and the call that makes both, which CALLS the public entry points one after another.
#include <cmath>

#include "last_frame.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {
namespace {

// The context's plane, Ctx::last_frame, made on first use and grown when more is asked for: 8 B per pixel
struct LastFrameWs {
    void* plane = nullptr;
    size_t bytes = 0;
};

int last_frame_plane(Ctx* c, size_t bytes, unsigned long long** out) {
    if (!c->last_frame) c->last_frame = new LastFrameWs();
    LastFrameWs* w = static_cast<LastFrameWs*>(c->last_frame);
    if (w->bytes < bytes) {
        if (w->plane) {
            RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
            RSDSFM_HIP_CHECK(c, hipFree(w->plane));
        }
        w->plane = nullptr, w->bytes = 0;
        RSDSFM_HIP_CHECK(c, hipMalloc(&w->plane, bytes));
        w->bytes = bytes;
    }
    *out = static_cast<unsigned long long*>(w->plane);
    return RSDSFM_OK;
}

bool finite3(const double* a) { return std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]); }

// what rsdsfm_advance_depth_dev refuses, as a message (NULL: nothing)
const char* advance_refusal(const double* d_field, const double* d_depth, const double* v3, const double* w3, double k, int rows, int cols, double fx, double fy,
                            double cx, double cy, double gamma, const double* d_out, const uint64_t* d_plane, const int64_t* d_count) {
    if (rows < 2 || cols < 2 || rows > 16384 || cols > 16384) return "advance depth: sides must be in [2, 16384]";
    if (!d_field || !d_depth || !v3 || !w3 || !d_out) return "advance depth: null pointer";
    const void* in[2] = {d_field, d_depth};
    const void* out[3] = {d_out, d_plane, d_count};
    for (int a = 0; a < 3; ++a) {
        if (!out[a]) continue;
        if (out[a] == in[0] || out[a] == in[1]) return "advance depth: an output is an input";
        for (int b = a + 1; b < 3; ++b)
            if (out[a] == out[b]) return "advance depth: two outputs share a buffer";
    }
    if (((uintptr_t)d_field | (uintptr_t)d_plane) & 15u) return "advance depth: the field and the plane must be 16-byte aligned";
    if ((uintptr_t)d_count & 7u) return "advance depth: the counter must be 8-byte aligned";
    if (!finite3(v3) || !finite3(w3) || !std::isfinite(k) || !std::isfinite(gamma)) return "advance depth: the motion and gamma must be finite";
    if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.0 || fy == 0.0 || !std::isfinite(cx) || !std::isfinite(cy) || gamma <= 0.0)
        return "advance depth: fx, fy must be finite and non-zero, cx, cy finite, gamma > 0";
    return nullptr;
}

}  // namespace

void last_frame_release(Ctx* c) {
    LastFrameWs* w = static_cast<LastFrameWs*>(c->last_frame);
    if (!w) return;
    if (w->plane) (void)hipFree(w->plane);
    delete w;
    c->last_frame = nullptr;
}

}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_advance_depth_launches(int32_t rows, int32_t cols) {
    if (rows < 2 || cols < 2 || rows > 16384 || cols > 16384) return RSDSFM_ERR_INVALID;
    return kAdvanceLaunches;
}

int rsdsfm_advance_depth_dev(rsdsfm_ctx* ctx, const double* d_field, const double* d_depth_colmajor, const double v3[3], const double w3[3], double k,
                             int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double gamma, int32_t global_shutter,
                             double* d_depth_out_colmajor, uint64_t* d_plane_or_null, int64_t* d_count_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (const char* why = advance_refusal(d_field, d_depth_colmajor, v3, w3, k, rows, cols, fx, fy, cx, cy, gamma, d_depth_out_colmajor, d_plane_or_null, d_count_or_null))
        return fail(c, RSDSFM_ERR_INVALID, why);
    unsigned long long* plane = reinterpret_cast<unsigned long long*>(d_plane_or_null);
    if (!plane) {
        const int rc = last_frame_plane(c, 8 * (size_t)rows * (size_t)cols, &plane);
        if (rc != RSDSFM_OK) return rc;
    }
    const LinkCamera cam{fx, fy, cx, cy, gamma, global_shutter ? 1 : 0};
    RSDSFM_HIP_CHECK(c, advance_depth_launch(c->stream, d_field, d_depth_colmajor, v3[2], w3[0], w3[1], k, cam, rows, cols, plane, d_depth_out_colmajor,
                                             reinterpret_cast<unsigned long long*>(d_count_or_null)));
    return RSDSFM_OK;
}

int rsdsfm_last_frame_motion(const double v3[3], const double w3[3], double k, double v_out3[3], double w_out3[3], double* k_out) {
    if (!v3 || !w3 || !v_out3 || !w_out3 || !k_out) return RSDSFM_ERR_INVALID;
    if (!finite3(v3) || !finite3(w3) || !std::isfinite(k) || !(1.0 + k > 0.0)) return RSDSFM_ERR_INVALID;
    const double f = (2.0 + 3.0 * k) / (2.0 + k);  // exactly 1 for k = 0
    const double kp = k / (1.0 + k);
    for (int i = 0; i < 3; ++i) {
        const double vi = v3[i] * f, wi = w3[i] * f;  // (the outputs may be the inputs)
        v_out3[i] = vi, w_out3[i] = wi;
    }
    *k_out = kp;
    return RSDSFM_OK;
}

int rsdsfm_last_frame_dev(rsdsfm_ctx* ctx, const double* d_field, const double* d_depth_colmajor, const double v3[3], const double w3[3], double k,
                          int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double gamma, int32_t global_shutter,
                          double* d_depth_out_colmajor, double* d_R_out, double* d_t_out, uint64_t* d_plane_or_null, int64_t* d_count_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    // everything any part refuses, before the first part enqueues
    if (const char* why = advance_refusal(d_field, d_depth_colmajor, v3, w3, k, rows, cols, fx, fy, cx, cy, gamma, d_depth_out_colmajor, d_plane_or_null, d_count_or_null))
        return fail(c, RSDSFM_ERR_INVALID, why);
    if (!d_R_out || !d_t_out) return fail(c, RSDSFM_ERR_INVALID, "last frame: null pose table");
    const void* others[5] = {d_field, d_depth_colmajor, d_depth_out_colmajor, d_plane_or_null, d_count_or_null};
    for (const void* o : others)
        if (o == d_R_out || o == d_t_out) return fail(c, RSDSFM_ERR_INVALID, "last frame: a pose table shares a buffer");
    if (d_R_out == d_t_out) return fail(c, RSDSFM_ERR_INVALID, "last frame: a pose table shares a buffer");
    double v2[3], w2[3], k2 = 0.0;
    if (rsdsfm_last_frame_motion(v3, w3, k, v2, w2, &k2) != RSDSFM_OK) return fail(c, RSDSFM_ERR_INVALID, "last frame: the motion needs 1 + k > 0");
    int rc = rsdsfm_advance_depth_dev(ctx, d_field, d_depth_colmajor, v3, w3, k, rows, cols, fx, fy, cx, cy, gamma, global_shutter, d_depth_out_colmajor, d_plane_or_null,
                                      d_count_or_null);
    if (rc != RSDSFM_OK) return rc;
    return rsdsfm_pose_table_dev(ctx, v2, w2, k2, gamma, rows, d_R_out, d_t_out);
}

}  // extern "C"
