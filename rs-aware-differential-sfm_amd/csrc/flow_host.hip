// flow_host.hip -- host driver of the DeepFlow front end and its single-pair C ABI (include/rsdsfm_flow.h; Camera::calculateDeepFlow,
// camera.cc:253-277).  One workspace type and one level loop serve single pairs (flow_kernels.hip) and batches of a
// clip (flow_seq_kernels.hip; the clip ABI is flow_seq_host.hip): pre-smoothing, pyramid, then per level (coarse to fine) one entry
// launch (upsample + warp + averaged image), one derivative launch, and per fixed-point iteration one coefficient launch + the SOR
// launches.  A batch of n pairs reads n + 1 frames and makes exactly the launches of one pair, each serving every pair of the batch
// (the boundary frame's pyramid is recomputed by the next batch: no extra launch).  All launches run on the context's stream.
#include <algorithm>
#include <cassert>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/rsdsfm_flow.h"
#include "flow_host.hpp"
#include "flow_kernels.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {
namespace flowhost {
namespace {

constexpr int kFlowMaxSide = 16384;

bool params_ok(const rsdsfm_flow_params& p) {
    const double d[] = {p.sigma, p.downscale, p.alpha, p.delta, p.gamma, p.omega};
    for (double x : d)
        if (!std::isfinite(x)) return false;
    return p.sigma >= 0.0 && p.sigma <= 16.0 && p.min_size >= 0 && p.downscale > 0.0 && p.downscale < 1.0 && p.fixed_point_iterations > 0 &&
           p.sor_iterations > 0 && p.alpha > 0.0 && p.delta >= 0.0 && p.gamma >= 0.0 && p.omega > 0.0 && p.omega < 2.0;
}

bool sides_ok(int rows, int cols) { return rows >= 2 && cols >= 2 && rows <= kFlowMaxSide && cols <= kFlowMaxSide; }

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

FlowResizeTab make_tab(const FlowWs& w, const AxisTab& x, const AxisTab& y) {
    return FlowResizeTab{w.d_ti + x.i0, w.d_ti + x.i1, w.d_ti + y.i0, w.d_ti + y.i1, w.d_tf + x.w0, w.d_tf + x.w1, w.d_tf + y.w0, w.d_tf + y.w1};
}

#define FLOW_LAUNCH(expr)                                                                                                  \
    do {                                                                                                                   \
        hipError_t _e = (expr);                                                                                            \
        if (_e != hipSuccess) {                                                                                            \
            c->err = std::string(w->pair ? "deep flow: " : "deep flow sequence: ") + #expr + ": " + hipGetErrorString(_e); \
            return RSDSFM_ERR_HIP;                                                                                         \
        }                                                                                                                  \
    } while (0)

}  // namespace

int check_args(Ctx* c, int rows, int cols, int channels, const rsdsfm_flow_params* pp, rsdsfm_flow_params* p) {
    if (!sides_ok(rows, cols)) return fail(c, RSDSFM_ERR_INVALID, "deep flow: sides must be in [2, 16384]");
    if (channels != 1 && channels != 3) return fail(c, RSDSFM_ERR_INVALID, "deep flow: channels must be 1 or 3");
    *p = pp ? *pp : defaults();
    if (!params_ok(*p)) return fail(c, RSDSFM_ERR_INVALID, "deep flow: bad parameters");
    return RSDSFM_OK;
}

FlowWs* flow_ws(Ctx* c, bool pair) {
    void*& slot = pair ? c->flow_pair : c->flow_clip;
    if (!slot) slot = new FlowWs(pair);
    return static_cast<FlowWs*>(slot);
}

int ensure_flow_ws(Ctx* c, FlowWs* w, int B, int rows, int cols, const rsdsfm_flow_params& p) {
    assert(B >= 1 && B <= kFlowSeqMaxPairs && (!w->pair || B == 1));
    if (w->d_buf && w->B == B && w->rows == rows && w->cols == cols && w->min_size == p.min_size && w->downscale == p.downscale && w->sigma == p.sigma)
        return RSDSFM_OK;
    if (w->d_buf || w->d_ring || w->d_tables) {
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // the previous batch may still read them
        if (w->d_buf) RSDSFM_HIP_CHECK(c, hipFree(w->d_buf));
        if (w->d_ring) RSDSFM_HIP_CHECK(c, hipFree(w->d_ring));
        if (w->d_tables) RSDSFM_HIP_CHECK(c, hipFree(w->d_tables));  // (rsdsfm_rectify_video_dev waits for every lane before it returns)
        w->d_buf = w->d_ring = nullptr;
        w->d_tables = nullptr;
    }
    w->B = w->rows = w->cols = 0;
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
    const size_t npix = (size_t)rows * cols;
    w->stride = Arena::need(4 * npix) / 4;  // (256-byte aligned planes)
    w->pstride = Arena::need(4 * total) / 4;
    const size_t pair_planes = 12 + 1 + FLOW_NDERIV + FLOW_NCOEF;  // two sets of six, avg, derivatives, coefficients
    static_assert(FLOW_NCOEF >= 2, "the coefficient block holds the B + 1 frames of the horizontal pass");
    // At B = 1 this is a single pair's 2 pyramids + 30 planes to the byte: 4 * pstride = Arena::need(4 * total) and 4 * stride =
    // Arena::need(4 * npix) are what Arena::take advances by for one pyramid / one plane, so a block of k of them is k separate slices.
    const size_t bytes = Arena::need(4 * w->ti.size()) + Arena::need(4 * w->tf.size()) + 4 * (size_t)(B + 1) * w->pstride +
                         4 * pair_planes * (size_t)B * w->stride;
    assert(B != 1 || bytes == Arena::need(4 * w->ti.size()) + Arena::need(4 * w->tf.size()) + 2 * Arena::need(4 * total) + pair_planes * Arena::need(4 * npix));
    RSDSFM_HIP_CHECK(c, hipMalloc(&w->d_buf, bytes));
    Arena a(w->d_buf);
    w->d_ti = a.take<int32_t>(w->ti.size());
    w->d_tf = a.take<float>(w->tf.size());
    w->pyr = a.take<float>((size_t)(B + 1) * w->pstride);
    for (int s = 0; s < 2; ++s)
        for (int k = 0; k < 6; ++k) w->set[s][k] = a.take<float>((size_t)B * w->stride);
    w->avg = a.take<float>((size_t)B * w->stride);
    for (int k = 0; k < FLOW_NDERIV; ++k) w->d[k] = a.take<float>((size_t)B * w->stride);
    float* cb = a.take<float>((size_t)FLOW_NCOEF * B * w->stride);
    for (int k = 0; k < FLOW_NCOEF; ++k) w->c[k] = cb + (size_t)k * B * w->stride;
    assert(a.off == bytes);
    if (!w->ti.empty()) RSDSFM_HIP_CHECK(c, hipMemcpyAsync(w->d_ti, w->ti.data(), 4 * w->ti.size(), hipMemcpyHostToDevice, c->stream));
    RSDSFM_HIP_CHECK(c, hipMemcpyAsync(w->d_tf, w->tf.data(), 4 * w->tf.size(), hipMemcpyHostToDevice, c->stream));
    RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // the host tables are pageable
    w->B = B, w->rows = rows, w->cols = cols, w->min_size = p.min_size, w->downscale = p.downscale, w->sigma = p.sigma;
    return RSDSFM_OK;
}

int flow_enqueue(Ctx* c, const FlowWs* w, const uint8_t* const* frames, int n, int channels, const rsdsfm_flow_params& p, double* const* flows) {
    assert(n >= 1 && n <= w->B);
    hipStream_t s = c->stream;
    const int nl = (int)w->lr.size();
    const size_t stride = w->stride, pstride = w->pstride;
    FlowFramePtrs fp{};
    for (int f = 0; f <= n; ++f) fp.p[f] = frames[f];
    FlowOutPtrs op{};
    for (int q = 0; q < n; ++q) op.p[q] = flows[q];
    // pre-smoothing (the coefficient block serves as the horizontal pass's output) and the pyramid
    if (w->pair)
        FLOW_LAUNCH(flow_presmooth(s, frames[0], frames[1], w->rows, w->cols, channels, w->d_tf, w->radius, w->c[0], w->c[0] + stride, w->pyr, w->pyr + pstride));
    else
        FLOW_LAUNCH(flow_seq_presmooth(s, fp, n + 1, w->rows, w->cols, channels, w->d_tf, w->radius, w->c[0], stride, w->pyr, pstride));
    for (int l = 0; l + 1 < nl; ++l) {
        const float* src = w->pyr + w->lvl_off[l];
        float* dst = w->pyr + w->lvl_off[l + 1];
        const FlowResizeTab tab = make_tab(*w, w->down_x[l], w->down_y[l]);
        if (w->pair)
            FLOW_LAUNCH(flow_pyr_down(s, src, src + pstride, w->lc[l], tab, w->lr[l + 1], w->lc[l + 1], dst, dst + pstride));
        else
            FLOW_LAUNCH(flow_seq_pyr_down(s, src, w->lc[l], tab, w->lr[l + 1], w->lc[l + 1], dst, pstride, n + 1));
    }
    const FlowConsts k{(float)(4.0 * p.alpha), (float)(p.delta / 3.0), (float)(p.gamma / 3.0)};
    const float scale = (float)(1.0 / p.downscale), om = (float)p.omega, om1 = (float)(1.0 - p.omega);
    int cur_prev = 0;  // which du / dv pair of the coarser level holds its increment
    for (int l = nl - 1; l >= 0; --l) {
        const int r = w->lr[l], cc = w->lc[l];
        float* const* S = w->set[l & 1];
        const float* pyr_l = w->pyr + w->lvl_off[l];
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
        if (w->pair)
            FLOW_LAUNCH(flow_level_entry(s, L, pyr_l, pyr_l + pstride, r, cc, C, scale));
        else
            FLOW_LAUNCH(flow_seq_level_entry(s, L, stride, pyr_l, pstride, r, cc, C, scale, n));
        // SOR geometry: one region without halo when the level fits, else regions of interior kFlowRegion - 2 halo (red-black order:
        // the tiling decides no value)
        const bool single = r <= kFlowRegion && cc <= kFlowRegion;
        const int halo = single ? 0 : 2 * kFlowSorBlock, inner = kFlowRegion - 2 * halo;
        const int tiles_x = (cc + inner - 1) / inner, tiles_y = (r + inner - 1) / inner;
        const int per_launch = single ? p.sor_iterations : kFlowSorBlock;
        int cur = 0;
        for (int f = 0; f < p.fixed_point_iterations; ++f) {
            L.du = S[2 + 2 * cur], L.dv = S[3 + 2 * cur];
            if (w->pair)
                FLOW_LAUNCH(flow_coef(s, L, r, cc, k));
            else
                FLOW_LAUNCH(flow_seq_coef(s, L, stride, r, cc, k, n));
            for (int done = 0; done < p.sor_iterations; done += per_launch) {
                FlowSorArgs a;
                for (int q = 0; q < FLOW_NCOEF; ++q) a.c[q] = w->c[q];
                a.du_in = S[2 + 2 * cur], a.dv_in = S[3 + 2 * cur];
                a.du_out = S[2 + 2 * (1 - cur)], a.dv_out = S[3 + 2 * (1 - cur)];
                a.rows = r, a.cols = cc, a.halo = halo, a.tiles_x = tiles_x;
                a.nit = std::min(per_launch, p.sor_iterations - done);
                a.om = om, a.om1 = om1;
                if (w->pair)
                    FLOW_LAUNCH(flow_sor(s, a, tiles_x * tiles_y));
                else
                    FLOW_LAUNCH(flow_seq_sor(s, a, stride, tiles_x * tiles_y, n));
                cur = 1 - cur;
            }
        }
        cur_prev = cur;
        if (l == 0) {
            L.du = S[2 + 2 * cur], L.dv = S[3 + 2 * cur];
            if (w->pair)
                FLOW_LAUNCH(flow_output(s, L, r, cc, flows[0]));
            else
                FLOW_LAUNCH(flow_seq_output(s, L, stride, r, cc, op, n));
        }
    }
    return RSDSFM_OK;
}

int flow_staged(Ctx* c, const FlowWs* w, const uint8_t* const* frames, int nframes, int channels, const rsdsfm_flow_params& p, double* const* flows) {
    const int B = w->B;
    const size_t npix = (size_t)w->rows * (size_t)w->cols, img_bytes = npix * (size_t)channels;
    int rc = ensure_stage(c, (size_t)(B + 1) * Arena::need(img_bytes) + (size_t)B * Arena::need(16 * npix));
    if (rc != RSDSFM_OK) return rc;
    Arena sa(c->d_stage);
    const uint8_t* d_img[kFlowSeqMaxPairs + 1];
    double* d_flow[kFlowSeqMaxPairs];
    for (int f = 0; f <= B; ++f) d_img[f] = sa.take<uint8_t>(img_bytes);
    for (int q = 0; q < B; ++q) d_flow[q] = sa.take<double>(2 * npix);
    for (int g0 = 0; g0 < nframes - 1; g0 += B) {
        const int n = std::min(B, nframes - 1 - g0);
        for (int f = 0; f <= n; ++f)
            RSDSFM_HIP_CHECK(c, hipMemcpyAsync(const_cast<uint8_t*>(d_img[f]), frames[g0 + f], img_bytes, hipMemcpyHostToDevice, c->stream));
        rc = flow_enqueue(c, w, d_img, n, channels, p, d_flow);
        if (rc != RSDSFM_OK) return rc;
        for (int q = 0; q < n; ++q) RSDSFM_HIP_CHECK(c, hipMemcpyAsync(flows[g0 + q], d_flow[q], 16 * npix, hipMemcpyDeviceToHost, c->stream));
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // the next batch overwrites the staging buffer
    }
    return RSDSFM_OK;
}

}  // namespace flowhost

void flow_release(Ctx* c) {
    for (void** slot : {&c->flow_pair, &c->flow_clip}) {
        flowhost::FlowWs* w = static_cast<flowhost::FlowWs*>(*slot);
        if (!w) continue;
        if (w->d_buf) (void)hipFree(w->d_buf);
        if (w->d_ring) (void)hipFree(w->d_ring);
        if (w->d_tables) (void)hipFree(w->d_tables);
        delete w;
        *slot = nullptr;
    }
}

}  // namespace rsdsfm

using namespace rsdsfm;
using namespace rsdsfm::flowhost;

extern "C" {

int rsdsfm_flow_default_params(rsdsfm_flow_params* out) {
    if (!out) return RSDSFM_ERR_INVALID;
    *out = defaults();
    return RSDSFM_OK;
}

int rsdsfm_flow_levels(int32_t rows, int32_t cols, const rsdsfm_flow_params* params_or_null, int32_t* n, int32_t* level_rows, int32_t* level_cols) {
    if (!n) return RSDSFM_ERR_INVALID;
    const rsdsfm_flow_params p = params_or_null ? *params_or_null : defaults();
    if (!sides_ok(rows, cols) || !params_ok(p)) return RSDSFM_ERR_INVALID;
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
    FlowWs* w = flow_ws(c, true);
    rc = ensure_flow_ws(c, w, 1, rows, cols, p);
    if (rc != RSDSFM_OK) return rc;
    const uint8_t* const frames[2] = {d_img1, d_img2};
    return flow_enqueue(c, w, frames, 1, channels, p, &d_flow);
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
    FlowWs* w = flow_ws(c, true);
    rc = ensure_flow_ws(c, w, 1, rows, cols, p);
    if (rc != RSDSFM_OK) return rc;
    const uint8_t* const frames[2] = {img1, img2};
    return flow_staged(c, w, frames, 2, channels, p, &flow);
}

}  // extern "C"
