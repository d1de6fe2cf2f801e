// link_host.hip -- C ABI of a clip's trajectory (include/rsdsfm_trajectory.h; tests/link_spec_numpy.py is the definition, link_kernels.hip
// the kernels): the links of solved pairs, the chain of scales and poses (host arithmetic), the clip's points, and the clip call that runs
// them behind rsdsfm_solve_video_dev / rsdsfm_solve_video_checked_dev.  No solve code of its own: the linked call CALLS the two entry points.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/rsdsfm_trajectory.h"
#include "link.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"

namespace rsdsfm {
namespace {

// The context's link workspace, Ctx::link, made on first use and grown when more is asked for:
struct LinkWs {
    void* planes = nullptr;  // ratio planes of the links in flight: 8 B per pixel per link
    size_t plane_bytes = 0;
    unsigned* hist = nullptr;    // kLinkMax x kLinkBins words: the links' histograms
    LinkState* state = nullptr;  // kLinkMax records
};

int link_ws(Ctx* c, size_t plane_bytes, LinkWs** out) {
    if (!c->link) c->link = new LinkWs();
    LinkWs* w = static_cast<LinkWs*>(c->link);
    if (!w->hist) RSDSFM_HIP_CHECK(c, hipMalloc(reinterpret_cast<void**>(&w->hist), sizeof(unsigned) * kLinkMax * kLinkBins));
    if (!w->state) RSDSFM_HIP_CHECK(c, hipMalloc(reinterpret_cast<void**>(&w->state), sizeof(LinkState) * kLinkMax));
    if (w->plane_bytes < plane_bytes) {
        if (w->planes) {
            RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
            RSDSFM_HIP_CHECK(c, hipFree(w->planes));
        }
        w->planes = nullptr, w->plane_bytes = 0;
        RSDSFM_HIP_CHECK(c, hipMalloc(&w->planes, plane_bytes));
        w->plane_bytes = plane_bytes;
    }
    *out = w;
    return RSDSFM_OK;
}

rsdsfm_link_params link_defaults() { return rsdsfm_link_params{0.1, 16, 0, (int32_t)sizeof(rsdsfm_link_params), 0}; }

int link_params(Ctx* c, const rsdsfm_link_params* pp, rsdsfm_link_params* p) {
    *p = pp ? *pp : link_defaults();
    if (p->struct_bytes != 0 && p->struct_bytes != (int32_t)sizeof(rsdsfm_link_params))
        return fail(c, RSDSFM_ERR_INVALID, "rsdsfm_link_params: struct_bytes is neither 0 nor sizeof(rsdsfm_link_params) -- caller built against another header (use rsdsfm_link_params_init)");
    if (!std::isfinite(p->tol) || p->tol < 0.0 || p->min_links < 0) return fail(c, RSDSFM_ERR_INVALID, "link: tol must be finite and >= 0, min_links >= 0");
    if (p->radix_bits != 0 && p->radix_bits != 8 && p->radix_bits != 11) return fail(c, RSDSFM_ERR_INVALID, "link: radix_bits must be 0 (default), 8 or 11");
    if (p->radix_bits == 0) p->radix_bits = kLinkMaxBits;
    return RSDSFM_OK;
}

// the links of npairs pairs, kLinkMax at a time; synchronous in the records
int link_run(Ctx* c, const double* const* d_fields, const double* const* d_maps, const double* v, const double* w, const double* k, int npairs, int rows,
             int cols, const LinkCamera& cam, const rsdsfm_link_params& p, uint64_t* const* d_planes, rsdsfm_link_record* records) {
    const int nlinks = npairs - 1;
    const size_t plane_stride = Arena::need(8 * (size_t)rows * (size_t)cols);
    LinkWs* ws = nullptr;
    int rc = link_ws(c, d_planes ? 0 : (size_t)std::min(nlinks, kLinkMax) * plane_stride, &ws);
    if (rc != RSDSFM_OK) return rc;
    std::vector<LinkState> host((size_t)std::min(nlinks, kLinkMax));
    for (int l0 = 0; l0 < nlinks; l0 += kLinkMax) {
        const int n = std::min(kLinkMax, nlinks - l0);
        LinkPtrs t{};
        LinkMotion m{};
        for (int l = 0; l < n; ++l) {
            const int q = l0 + l;
            t.field[l] = d_fields[q], t.zp[l] = d_maps[q], t.zn[l] = d_maps[q + 1];
            t.plane[l] = d_planes ? reinterpret_cast<unsigned long long*>(d_planes[q])
                                  : reinterpret_cast<unsigned long long*>(static_cast<char*>(ws->planes) + (size_t)l * plane_stride);
            m.v2[l] = v[3 * q + 2], m.w0[l] = w[3 * q], m.w1[l] = w[3 * q + 1], m.k[l] = k[q];
        }
        RSDSFM_HIP_CHECK(c, hipMemsetAsync(ws->hist, 0, sizeof(unsigned) * (size_t)n * kLinkBins, c->stream));
        RSDSFM_HIP_CHECK(c, hipMemsetAsync(ws->state, 0, sizeof(LinkState) * (size_t)n, c->stream));
        RSDSFM_HIP_CHECK(c, link_launch(c->stream, t, m, cam, n, rows, cols, p.radix_bits, p.tol, ws->hist, ws->state));
        RSDSFM_HIP_CHECK(c, hipMemcpyAsync(host.data(), ws->state, sizeof(LinkState) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        for (int l = 0; l < n; ++l) {
            rsdsfm_link_record& r = records[l0 + l];
            r.n = (int64_t)host[l].n, r.agree = (int64_t)host[l].agree, r.reserved = 0;
            r.valid = r.n >= (int64_t)p.min_links ? 1 : 0;
            if (r.n > 0) {
                static_assert(sizeof(double) == sizeof(unsigned long long), "bit pattern of a double");
                std::memcpy(&r.ratio, &host[l].prefix, sizeof(double));
            } else {
                r.ratio = std::numeric_limits<double>::quiet_NaN();
            }
        }
    }
    return RSDSFM_OK;
}

int check_link_args(Ctx* c, int npairs, int rows, int cols, double fx, double fy, double gamma) {
    if (npairs < 2) return fail(c, RSDSFM_ERR_INVALID, "link: npairs must be >= 2");
    if (rows < 2 || cols < 2 || rows > 16384 || cols > 16384) return fail(c, RSDSFM_ERR_INVALID, "link: sides must be in [2, 16384]");
    if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.0 || fy == 0.0 || !std::isfinite(gamma) || gamma <= 0.0)
        return fail(c, RSDSFM_ERR_INVALID, "link: fx, fy must be finite and non-zero, gamma finite and > 0");
    return RSDSFM_OK;
}

// exp([a]x) = I + sin(t) / t [a]x + (1 - cos(t)) / t^2 [a]x^2 (row-major); the series' first terms below t = 1e-8
void rodrigues(const double a[3], double R[9]) {
    const double t2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    const double t = std::sqrt(t2);
    double s, cc;
    if (t < 1e-8)
        s = 1.0 - t2 / 6.0, cc = 0.5 - t2 / 24.0;
    else
        s = std::sin(t) / t, cc = (1.0 - std::cos(t)) / t2;
    const double X[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double xx = (X[i * 3] * X[j] + X[i * 3 + 1] * X[3 + j]) + X[i * 3 + 2] * X[6 + j];
            R[i * 3 + j] = ((i == j ? 1.0 : 0.0) + s * X[i * 3 + j]) + cc * xx;
        }
}

int points_run(Ctx* c, const float* const* in, float* const* out, int npairs, int rows, int cols, const double* scales, const double* A, const double* cc) {
    const int64_t npix = (int64_t)rows * cols;
    for (int q0 = 0; q0 < npairs; q0 += kPointsMax) {
        const int n = std::min(kPointsMax, npairs - q0);
        PointsArgs a{};
        for (int l = 0; l < n; ++l) {
            const int q = q0 + l;
            a.in[l] = in[q], a.out[l] = out[q], a.scale[l] = scales[q];
            std::copy(A + 9 * (size_t)q, A + 9 * (size_t)q + 9, a.A[l]);
            std::copy(cc + 3 * (size_t)q, cc + 3 * (size_t)q + 3, a.c[l]);
        }
        RSDSFM_HIP_CHECK(c, clip_points_launch(c->stream, a, n, npix));
    }
    return RSDSFM_OK;
}

int check_points_args(Ctx* c, const float* const* in, float* const* out, int npairs, int rows, int cols) {
    if (npairs < 1) return fail(c, RSDSFM_ERR_INVALID, "clip points: npairs must be >= 1");
    if (rows < 2 || cols < 2 || rows > 16384 || cols > 16384) return fail(c, RSDSFM_ERR_INVALID, "clip points: sides must be in [2, 16384]");
    if (!all_set(in, npairs) || !all_set(out, npairs)) return fail(c, RSDSFM_ERR_INVALID, "clip points: null device pointer");
    for (int a = 0; a < npairs; ++a)
        for (int b = 0; b < npairs; ++b)
            if ((a != b && (out[a] == out[b] || out[a] == in[b]))) return fail(c, RSDSFM_ERR_INVALID, "clip points: an output is another pair's buffer");
    return RSDSFM_OK;
}

}  // namespace

void link_rodrigues(const double a[3], double R[9]) { rodrigues(a, R); }

void link_release(Ctx* c) {
    LinkWs* w = static_cast<LinkWs*>(c->link);
    if (!w) return;
    if (w->planes) (void)hipFree(w->planes);
    if (w->hist) (void)hipFree(w->hist);
    if (w->state) (void)hipFree(w->state);
    delete w;
    c->link = nullptr;
}

}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_link_params_init(rsdsfm_link_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = link_defaults();
    return RSDSFM_OK;
}

int rsdsfm_link_pairs_dev(rsdsfm_ctx* ctx, const double* const* d_fields, const double* const* d_depth_maps, const double* v_3n, const double* w_3n,
                          const double* k_n, int32_t npairs, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double gamma,
                          int32_t global_shutter, const rsdsfm_link_params* params_or_null, uint64_t* const* d_ratio_planes_or_null,
                          rsdsfm_link_record* records) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = check_link_args(c, npairs, rows, cols, fx, fy, gamma);
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_link_params p;
    rc = link_params(c, params_or_null, &p);
    if (rc != RSDSFM_OK) return rc;
    if (!v_3n || !w_3n || !k_n || !records) return fail(c, RSDSFM_ERR_INVALID, "link: null pointer");
    if (!all_set(d_fields, npairs - 1) || !all_set(d_depth_maps, npairs) || (d_ratio_planes_or_null && !all_set(d_ratio_planes_or_null, npairs - 1)))
        return fail(c, RSDSFM_ERR_INVALID, "link: null device pointer");
    if (d_ratio_planes_or_null)
        for (int a = 0; a < npairs - 1; ++a) {
            const void* pl = d_ratio_planes_or_null[a];
            for (int b = 0; b < npairs; ++b)
                if (pl == d_depth_maps[b] || (b < npairs - 1 && (pl == d_fields[b] || (b != a && pl == d_ratio_planes_or_null[b]))))
                    return fail(c, RSDSFM_ERR_INVALID, "link: a ratio plane is an input or another link's plane");
        }
    const LinkCamera cam{fx, fy, cx, cy, gamma, global_shutter ? 1 : 0};
    return link_run(c, d_fields, d_depth_maps, v_3n, w_3n, k_n, npairs, rows, cols, cam, p, d_ratio_planes_or_null, records);
}

int rsdsfm_chain_clip(const rsdsfm_link_record* records, const double* v_3n, const double* w_3n, int32_t npairs, double gamma, double* scales, double* A,
                      double* c, uint8_t* broken_or_null) {
    if (npairs < 1 || !v_3n || !w_3n || !scales || !A || !c || (npairs > 1 && !records) || !std::isfinite(gamma) || gamma <= 0.0) return RSDSFM_ERR_INVALID;
    scales[0] = 1.0;
    for (int q = 0; q + 1 < npairs; ++q) {
        const double r = records[q].ratio;
        const bool good = records[q].valid && std::isfinite(r) && r > 0.0;
        scales[q + 1] = good ? scales[q] / r : scales[q];
        if (broken_or_null) broken_or_null[q] = good ? 0 : 1;
    }
    for (int i = 0; i < 9; ++i) A[i] = (i % 4 == 0) ? 1.0 : 0.0;
    c[0] = c[1] = c[2] = 0.0;
    for (int q = 0; q < npairs; ++q) {
        const double a[3] = {w_3n[3 * q] / gamma, w_3n[3 * q + 1] / gamma, w_3n[3 * q + 2] / gamma};
        double R[9];
        rodrigues(a, R);
        const double* Aq = A + 9 * (size_t)q;
        double* An = A + 9 * (size_t)(q + 1);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) An[i * 3 + j] = (Aq[i * 3] * R[j * 3] + Aq[i * 3 + 1] * R[j * 3 + 1]) + Aq[i * 3 + 2] * R[j * 3 + 2];  // A_q R_q^T
        const double s = scales[q];
        const double d[3] = {s * v_3n[3 * q] / gamma, s * v_3n[3 * q + 1] / gamma, s * v_3n[3 * q + 2] / gamma};
        for (int i = 0; i < 3; ++i) c[3 * (size_t)(q + 1) + i] = c[3 * (size_t)q + i] - ((An[i * 3] * d[0] + An[i * 3 + 1] * d[1]) + An[i * 3 + 2] * d[2]);
    }
    return RSDSFM_OK;
}

int rsdsfm_clip_points_dev(rsdsfm_ctx* ctx, const float* const* d_points_in, float* const* d_points_out, int32_t npairs, int32_t rows, int32_t cols,
                           const double* scales, const double* A, const double* c_) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    int rc = check_points_args(c, d_points_in, d_points_out, npairs, rows, cols);
    if (rc != RSDSFM_OK) return rc;
    if (!scales || !A || !c_) return fail(c, RSDSFM_ERR_INVALID, "clip points: null pointer");
    return points_run(c, d_points_in, d_points_out, npairs, rows, cols, scales, A, c_);
}

int rsdsfm_solve_video_linked_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                  double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                  const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows, double* const* d_depth_maps,
                                  double* const* d_R_or_null, double* const* d_t_or_null, rsdsfm_frame_result* results,
                                  const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks_or_null,
                                  const rsdsfm_link_params* link_params_or_null, rsdsfm_link_record* records, double* scales, double* A, double* c_,
                                  uint8_t* broken_or_null, float* const* d_points_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (!d_flows)
        return fail(c, RSDSFM_ERR_INVALID,
                    "solve video linked: d_flows is required -- the library's ring keeps only B fields, and link p reads pair p's field after pair p + 1 is solved");
    rsdsfm_link_params p;
    int rc = link_params(c, link_params_or_null, &p);
    if (rc != RSDSFM_OK) return rc;
    const int np = nframes - 1;
    if (!scales || !A || !c_ || (np > 1 && !records)) return fail(c, RSDSFM_ERR_INVALID, "solve video linked: null pointer");
    if (np >= 1 && d_points_or_null) {
        rc = check_points_args(c, d_points_or_null, d_points_or_null, np, rows, cols);
        if (rc != RSDSFM_OK) return rc;
    }
    // the solve: the public entry point itself, so that it runs the code it runs alone
    rc = d_masks_or_null ? rsdsfm_solve_video_checked_dev(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds,
                                                          d_flows, d_depth_maps, d_R_or_null, d_t_or_null, results, check_params_or_null, d_masks_or_null,
                                                          nullptr, nullptr)
                         : rsdsfm_solve_video_dev(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds,
                                                  d_flows, d_depth_maps, d_R_or_null, d_t_or_null, results);
    if (rc != RSDSFM_OK) return rc;
    std::vector<double> v(3 * (size_t)np), w(3 * (size_t)np), k((size_t)np);
    for (int q = 0; q < np; ++q) {
        std::copy(results[q].v, results[q].v + 3, v.begin() + 3 * q);
        std::copy(results[q].w, results[q].w + 3, w.begin() + 3 * q);
        k[q] = results[q].k;
    }
    if (np >= 2) {
        rc = check_link_args(c, np, rows, cols, fx, fy, gamma);
        if (rc != RSDSFM_OK) return rc;
        const LinkCamera cam{fx, fy, cx, cy, gamma, params->use_global_shutter_mode ? 1 : 0};
        rc = link_run(c, d_flows, d_depth_maps, v.data(), w.data(), k.data(), np, rows, cols, cam, p, nullptr, records);
        if (rc != RSDSFM_OK) return rc;
    }
    if (rsdsfm_chain_clip(records, v.data(), w.data(), np, gamma, scales, A, c_, broken_or_null) != RSDSFM_OK)
        return fail(c, RSDSFM_ERR_INVALID, "solve video linked: gamma must be finite and > 0");
    if (d_points_or_null) return points_run(c, d_points_or_null, d_points_or_null, np, rows, cols, scales, A, c_);
    return RSDSFM_OK;
}

}  // extern "C"
