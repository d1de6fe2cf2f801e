// flow_host.hip -- C ABI of the DeepFlow front end (include/rsdsfm_flow.h; Camera::calculateDeepFlow, camera.cc:253-277; DESIGN
// section 12).  Drives flow_kernels.hip: pre-smoothing, pyramid, then per level (coarse to fine) one entry launch (upsample + warp +
// averaged image), one derivative launch, and per fixed-point iteration one coefficient launch + the SOR launches.
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/rsdsfm_flow.h"
#include "flow_host.hpp"
#include "flow_kernels.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {
namespace flowhost {

bool params_ok(const rsdsfm_flow_params& p) {
    const double d[] = {p.sigma, p.downscale, p.alpha, p.delta, p.gamma, p.omega};
    for (double x : d)
        if (!std::isfinite(x)) return false;
    return p.sigma >= 0.0 && p.sigma <= 16.0 && p.min_size >= 0 && p.downscale > 0.0 && p.downscale < 1.0 && p.fixed_point_iterations > 0 &&
           p.sor_iterations > 0 && p.alpha > 0.0 && p.delta >= 0.0 && p.gamma >= 0.0 && p.omega > 0.0 && p.omega < 2.0;
}

rsdsfm_flow_params defaults() {
    rsdsfm_flow_params p;
    p.sigma = 0.6;
    p.min_size = 25;
    p.downscale = 0.95;
    p.fixed_point_iterations = 5;
    p.sor_iterations = 25;
    p.alpha = 1.0;
    p.delta = 0.5;
    p.gamma = 5.0;
    p.omega = 1.6;
    return p;
}

void levels_of(int rows, int cols, const rsdsfm_flow_params& p, std::vector<int>& lr, std::vector<int>& lc) {
    lr.assign(1, rows);
    lc.assign(1, cols);
    for (;;) {
        const int r = lr.back(), c = lc.back();
        const int nr = (int)(r * p.downscale + 0.5), nc = (int)(c * p.downscale + 0.5);
        // no level with a side below 2: a 1x1 level has no neighbour and no derivative, its system is 0 * du = 0 (R1 = 1 / 0)
        if (nr <= p.min_size || nc <= p.min_size || nr < 2 || nc < 2 || (nr == r && nc == c)) return;
        lr.push_back(nr);
        lc.push_back(nc);
    }
}

std::vector<float> gauss_taps(double sigma) {
    const int r = (int)std::floor(3.0 * sigma);
    if (r <= 0) return {1.0f};
    std::vector<double> g;
    double s = 0.0;
    for (int i = -r; i <= r; ++i) {
        g.push_back(std::exp(-(double)(i * i) / (2.0 * sigma * sigma)));
        s += g.back();
    }
    std::vector<float> t;
    for (double x : g) t.push_back((float)(x / s));
    return t;
}

AxisTab axis_table(int src, int dst, std::vector<int32_t>& ti, std::vector<float>& tf) {
    AxisTab a{ti.size(), ti.size() + (size_t)dst, tf.size(), tf.size() + (size_t)dst};
    std::vector<int32_t> i0(dst), i1(dst);
    std::vector<float> w0(dst), w1(dst);
    for (int d = 0; d < dst; ++d) {
        double fx = ((double)d + 0.5) * (double)src / (double)dst - 0.5;
        fx = std::min(std::max(fx, 0.0), (double)(src - 1));
        const int x = (int)std::floor(fx);
        const double t = fx - x;
        i0[d] = x;
        i1[d] = std::min(x + 1, src - 1);
        w0[d] = (float)(1.0 - t);
        w1[d] = (float)t;
    }
    ti.insert(ti.end(), i0.begin(), i0.end());
    ti.insert(ti.end(), i1.begin(), i1.end());
    tf.insert(tf.end(), w0.begin(), w0.end());
    tf.insert(tf.end(), w1.begin(), w1.end());
    return a;
}

int check_args(Ctx* c, int rows, int cols, int channels, const rsdsfm_flow_params* pp, rsdsfm_flow_params* p) {
    if (rows < 2 || cols < 2 || rows > kFlowMaxSide || cols > kFlowMaxSide) return fail(c, RSDSFM_ERR_INVALID, "deep flow: sides must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "deep flow: channels must be 1 or 3");
    *p = pp ? *pp : defaults();
    if (!params_ok(*p)) return fail(c, RSDSFM_ERR_INVALID, "deep flow: bad parameters");
    return RSDSFM_OK;
}

}  // namespace flowhost

using namespace flowhost;

namespace {

// the context's pyramid workspace: one device allocation, rebuilt when the size or the pyramid changes
struct FlowWs {
    int rows = 0, cols = 0, min_size = -1;
    double downscale = 0.0, sigma = -1.0;
    void* d_buf = nullptr;
    size_t bytes = 0;
    std::vector<int> lr, lc;
    std::vector<size_t> lvl_off;  // pyramid level offsets (floats) into each image's pyramid
    std::vector<AxisTab> down_x, down_y, up_x, up_y;  // [l]: level l -> l + 1 / level l + 1 -> l
    int radius = 0;
    std::vector<int32_t> ti;
    std::vector<float> tf;  // taps first, then the resize weights
    // device pointers
    int32_t* d_ti = nullptr;
    float* d_tf = nullptr;
    float *pyr1 = nullptr, *pyr2 = nullptr;
    float* set[2][6] = {};  // per level parity: u, v, du0, dv0, du1, dv1
    float* avg = nullptr;
    float* d[FLOW_NDERIV] = {};
    float* c[FLOW_NCOEF] = {};
};

std::mutex g_ws_mutex;
std::map<const Ctx*, FlowWs*> g_ws;

FlowResizeTab make_tab(const FlowWs& w, const AxisTab& x, const AxisTab& y) {
    return FlowResizeTab{w.d_ti + x.i0, w.d_ti + x.i1, w.d_ti + y.i0, w.d_ti + y.i1, w.d_tf + x.w0, w.d_tf + x.w1, w.d_tf + y.w0, w.d_tf + y.w1};
}

int ensure_flow_ws(Ctx* c, int rows, int cols, const rsdsfm_flow_params& p, FlowWs** out) {
    FlowWs* w;
    {
        std::lock_guard<std::mutex> lk(g_ws_mutex);
        FlowWs*& slot = g_ws[c];
        if (!slot) slot = new FlowWs();
        w = slot;
    }
    *out = w;
    if (w->d_buf && w->rows == rows && w->cols == cols && w->min_size == p.min_size && w->downscale == p.downscale && w->sigma == p.sigma) return RSDSFM_OK;
    if (w->d_buf) {
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // the previous pair may still read it
        RSDSFM_HIP_CHECK(c, hipFree(w->d_buf));
        w->d_buf = nullptr;
    }
    w->rows = w->cols = 0;
    levels_of(rows, cols, p, w->lr, w->lc);
    const int nl = (int)w->lr.size();
    w->ti.clear();
    w->tf = gauss_taps(p.sigma);
    w->radius = (int)w->tf.size() / 2;
    w->down_x.clear(), w->down_y.clear(), w->up_x.clear(), w->up_y.clear();
    w->lvl_off.assign(nl, 0);
    size_t total = 0;
    for (int l = 0; l < nl; ++l) {
        w->lvl_off[l] = total;
        total += (size_t)w->lr[l] * w->lc[l];
        if (l + 1 < nl) {
            w->down_x.push_back(axis_table(w->lc[l], w->lc[l + 1], w->ti, w->tf));
            w->down_y.push_back(axis_table(w->lr[l], w->lr[l + 1], w->ti, w->tf));
            w->up_x.push_back(axis_table(w->lc[l + 1], w->lc[l], w->ti, w->tf));
            w->up_y.push_back(axis_table(w->lr[l + 1], w->lr[l], w->ti, w->tf));
        }
    }
    const size_t n = (size_t)rows * cols;
    const size_t planes = 12 + 1 + FLOW_NDERIV + FLOW_NCOEF;  // two sets of six, avg, derivatives, coefficients
    size_t bytes = Arena::need(4 * w->ti.size()) + Arena::need(4 * w->tf.size()) + 2 * Arena::need(4 * total) + planes * Arena::need(4 * n);
    RSDSFM_HIP_CHECK(c, hipMalloc(&w->d_buf, bytes));
    w->bytes = bytes;
    Arena a(w->d_buf);
    w->d_ti = a.take<int32_t>(w->ti.size());
    w->d_tf = a.take<float>(w->tf.size());
    w->pyr1 = a.take<float>(total);
    w->pyr2 = a.take<float>(total);
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 6; ++k) w->set[s][k] = a.take<float>(n);
    w->avg = a.take<float>(n);
    for (int k = 0; k < FLOW_NDERIV; ++k) w->d[k] = a.take<float>(n);
    for (int k = 0; k < FLOW_NCOEF; ++k) w->c[k] = a.take<float>(n);
    if (!w->ti.empty()) RSDSFM_HIP_CHECK(c, hipMemcpyAsync(w->d_ti, w->ti.data(), 4 * w->ti.size(), hipMemcpyHostToDevice, c->stream));
    RSDSFM_HIP_CHECK(c, hipMemcpyAsync(w->d_tf, w->tf.data(), 4 * w->tf.size(), hipMemcpyHostToDevice, c->stream));
    RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // the host tables are pageable
    w->rows = rows, w->cols = cols, w->min_size = p.min_size, w->downscale = p.downscale, w->sigma = p.sigma;
    return RSDSFM_OK;
}

#define FLOW_LAUNCH(expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            c->err = std::string("deep flow: ") + #expr + ": " + hipGetErrorString(_e);          \
            return RSDSFM_ERR_HIP;                                                                 \
        }                                                                                          \
    } while (0)

int deep_flow_enqueue(Ctx* c, const uint8_t* img1, const uint8_t* img2, int rows, int cols, int channels, const rsdsfm_flow_params& p, double* flow) {
    FlowWs* w = nullptr;
    int rc = ensure_flow_ws(c, rows, cols, p, &w);
    if (rc != RSDSFM_OK) return rc;
    hipStream_t s = c->stream;
    const int nl = (int)w->lr.size();
    // pre-smoothing (the coefficient planes serve as the horizontal pass's output) and the pyramid
    FLOW_LAUNCH(flow_presmooth(s, img1, img2, rows, cols, channels, w->d_tf, w->radius, w->c[0], w->c[1], w->pyr1, w->pyr2));
    for (int l = 0; l + 1 < nl; ++l)
        FLOW_LAUNCH(flow_pyr_down(s, w->pyr1 + w->lvl_off[l], w->pyr2 + w->lvl_off[l], w->lc[l], make_tab(*w, w->down_x[l], w->down_y[l]), w->lr[l + 1],
                                  w->lc[l + 1], w->pyr1 + w->lvl_off[l + 1], w->pyr2 + w->lvl_off[l + 1]));
    const FlowConsts k{(float)(4.0 * p.alpha), (float)(p.delta / 3.0), (float)(p.gamma / 3.0)};
    const float scale = (float)(1.0 / p.downscale), om = (float)p.omega, om1 = (float)(1.0 - p.omega);
    int cur_prev = 0;  // which du / dv pair of the coarser level holds its increment
    for (int l = nl - 1; l >= 0; --l) {
        const int r = w->lr[l], cc = w->lc[l];
        float* const* S = w->set[l & 1];
        FlowLevelBufs L;
        L.u = S[0], L.v = S[1], L.du = S[2], L.dv = S[3], L.avg = w->avg;
        for (int q = 0; q < FLOW_NDERIV; ++q) L.d[q] = w->d[q];
        for (int q = 0; q < FLOW_NCOEF; ++q) L.c[q] = w->c[q];
        FlowCoarse C{};
        if (l + 1 < nl) {
            float* const* P = w->set[(l + 1) & 1];
            C.u = P[0], C.v = P[1], C.du = P[2 + 2 * cur_prev], C.dv = P[3 + 2 * cur_prev];
            C.rows = w->lr[l + 1], C.cols = w->lc[l + 1];
            C.tab = make_tab(*w, w->up_x[l], w->up_y[l]);
        }
        FLOW_LAUNCH(flow_level_entry(s, L, w->pyr1 + w->lvl_off[l], w->pyr2 + w->lvl_off[l], r, cc, C, scale));
        // SOR geometry: one region without halo when the level fits, else regions of interior kFlowRegion - 2 halo
        const bool single = r <= kFlowRegion && cc <= kFlowRegion;
        const int halo = single ? 0 : 2 * kFlowSorBlock, inner = kFlowRegion - 2 * halo;
        const int tiles_x = (cc + inner - 1) / inner, tiles_y = (r + inner - 1) / inner;
        const int per_launch = single ? p.sor_iterations : kFlowSorBlock;
        int cur = 0;
        for (int f = 0; f < p.fixed_point_iterations; ++f) {
            L.du = S[2 + 2 * cur], L.dv = S[3 + 2 * cur];
            FLOW_LAUNCH(flow_coef(s, L, r, cc, k));
            for (int done = 0; done < p.sor_iterations; done += per_launch) {
                FlowSorArgs a;
                for (int q = 0; q < FLOW_NCOEF; ++q) a.c[q] = w->c[q];
                a.du_in = S[2 + 2 * cur], a.dv_in = S[3 + 2 * cur];
                a.du_out = S[2 + 2 * (1 - cur)], a.dv_out = S[3 + 2 * (1 - cur)];
                a.rows = r, a.cols = cc, a.halo = halo, a.tiles_x = tiles_x;
                a.nit = std::min(per_launch, p.sor_iterations - done);
                a.om = om, a.om1 = om1;
                FLOW_LAUNCH(flow_sor(s, a, tiles_x * tiles_y));
                cur = 1 - cur;
            }
        }
        cur_prev = cur;
        if (l == 0) {
            L.du = S[2 + 2 * cur], L.dv = S[3 + 2 * cur];
            FLOW_LAUNCH(flow_output(s, L, r, cc, flow));
        }
    }
    return RSDSFM_OK;
}

}  // namespace

void flow_release(Ctx* c) {
    FlowWs* w = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_ws_mutex);
        auto it = g_ws.find(c);
        if (it == g_ws.end()) return;
        w = it->second;
        g_ws.erase(it);
    }
    if (w->d_buf) (void)hipFree(w->d_buf);
    delete w;
}

}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_flow_default_params(rsdsfm_flow_params* out) {
    if (!out) return RSDSFM_ERR_INVALID;
    *out = defaults();
    return RSDSFM_OK;
}

int rsdsfm_flow_levels(int32_t rows, int32_t cols, const rsdsfm_flow_params* params_or_null, int32_t* n, int32_t* level_rows, int32_t* level_cols) {
    if (!n) return RSDSFM_ERR_INVALID;
    const rsdsfm_flow_params p = params_or_null ? *params_or_null : defaults();
    if (rows < 2 || cols < 2 || rows > kFlowMaxSide || cols > kFlowMaxSide || !params_ok(p)) return RSDSFM_ERR_INVALID;
    std::vector<int> lr, lc;
    levels_of(rows, cols, p, lr, lc);
    const int cap = *n;
    *n = (int32_t)lr.size();
    if (!level_rows && !level_cols) return RSDSFM_OK;
    if (!level_rows || !level_cols || cap < (int)lr.size()) return RSDSFM_ERR_INVALID;
    for (size_t i = 0; i < lr.size(); ++i) level_rows[i] = lr[i], level_cols[i] = lc[i];
    return RSDSFM_OK;
}

int rsdsfm_deep_flow_dev(rsdsfm_ctx* ctx, const uint8_t* d_img1, const uint8_t* d_img2, int32_t rows, int32_t cols, int32_t channels,
                         const rsdsfm_flow_params* params_or_null, double* d_flow) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    rsdsfm_flow_params p;
    int rc = check_args(c, rows, cols, channels, params_or_null, &p);
    if (rc != RSDSFM_OK) return rc;
    if (!d_img1 || !d_img2 || !d_flow) return fail(c, RSDSFM_ERR_INVALID, "deep flow: null device pointer");
    return deep_flow_enqueue(c, d_img1, d_img2, rows, cols, channels, p, d_flow);
}

int rsdsfm_deep_flow(rsdsfm_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int32_t rows, int32_t cols, int32_t channels,
                     const rsdsfm_flow_params* params_or_null, double* flow) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    rsdsfm_flow_params p;
    int rc = check_args(c, rows, cols, channels, params_or_null, &p);
    if (rc != RSDSFM_OK) return rc;
    if (!img1 || !img2 || !flow) return fail(c, RSDSFM_ERR_INVALID, "deep flow: null pointer");
    const size_t npix = (size_t)rows * (size_t)cols, img_bytes = npix * (size_t)channels;
    rc = ensure_stage(c, 2 * Arena::need(img_bytes) + Arena::need(16 * npix));
    if (rc != RSDSFM_OK) return rc;
    Arena sa(c->d_stage);
    uint8_t* d_a = sa.take<uint8_t>(img_bytes);
    uint8_t* d_b = sa.take<uint8_t>(img_bytes);
    double* d_flow = sa.take<double>(2 * npix);
    RSDSFM_HIP_CHECK(c, hipMemcpyAsync(d_a, img1, img_bytes, hipMemcpyHostToDevice, c->stream));
    RSDSFM_HIP_CHECK(c, hipMemcpyAsync(d_b, img2, img_bytes, hipMemcpyHostToDevice, c->stream));
    rc = deep_flow_enqueue(c, d_a, d_b, rows, cols, channels, p, d_flow);
    if (rc != RSDSFM_OK) return rc;
    RSDSFM_HIP_CHECK(c, hipMemcpyAsync(flow, d_flow, 16 * npix, hipMemcpyDeviceToHost, c->stream));
    RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return RSDSFM_OK;
}

}  // extern "C"
