// flow_seq_host.hip -- C ABI of whole clips (include/rsdsfm_video.h; Camera::calculateDeepFlow, camera.cc:253-277, for every
// consecutive pair, and the solve of main.cc:380-457 per pair; DESIGN section 12, "Sequences").  Drives flow_seq_kernels.hip batch by
// batch: a batch of n <= B pairs reads n + 1 frames and makes exactly the launches of one pair of flow_host.hip, each serving every
// pair of the batch (the boundary frame's pyramid is recomputed by the next batch: no extra launch).  All launches run on the
// context's stream.
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rsdsfm_video.h"
#include "flow_host.hpp"
#include "flow_kernels.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {
namespace {

using namespace flowhost;

constexpr int kFlowBatchDefault = 8;  // profiles/flow_seq_time.txt

// The context's sequence workspace, separate from the single-pair one (alternating calls rebuild neither): one device allocation
// with the resize tables, B + 1 frame pyramids and B pairs' working planes, rebuilt when the size, the pyramid or B changes.  The
// ring of B fields of rsdsfm_solve_video_dev is a second allocation, made on first use.
struct FlowSeqWs {
    int batch = 0;  // rsdsfm_set_flow_batch; 0 = kFlowBatchDefault
    int B = 0, rows = 0, cols = 0, min_size = -1;
    double downscale = 0.0, sigma = -1.0;
    void* d_buf = nullptr;
    void* d_ring = nullptr;
    size_t ring_stride = 0;  // bytes between the ring's fields
    std::vector<int> lr, lc;
    std::vector<size_t> lvl_off;  // pyramid level offsets (floats) into each frame's pyramid
    std::vector<AxisTab> down_x, down_y, up_x, up_y;
    int radius = 0;
    std::vector<int32_t> ti;
    std::vector<float> tf;  // taps first, then the resize weights
    size_t stride = 0, pstride = 0;  // floats from one pair's plane to the next / from one frame's pyramid to the next
    int32_t* d_ti = nullptr;
    float* d_tf = nullptr;
    float* pyr = nullptr;   // B + 1 pyramids
    float* set[2][6] = {};  // per level parity: u, v, du0, dv0, du1, dv1 (B planes each)
    float* avg = nullptr;
    float* d[FLOW_NDERIV] = {};
    float* c[FLOW_NCOEF] = {};  // one block: the pre-smoothing's horizontal pass of the B + 1 frames uses it first
};

std::mutex g_seq_mutex;
std::map<const Ctx*, FlowSeqWs*> g_seq;

FlowSeqWs* seq_ws_of(const Ctx* c) {
    std::lock_guard<std::mutex> lk(g_seq_mutex);
    FlowSeqWs*& slot = g_seq[c];
    if (!slot) slot = new FlowSeqWs();
    return slot;
}

int batch_of(const FlowSeqWs* w) { return w->batch > 0 ? w->batch : kFlowBatchDefault; }

FlowResizeTab make_tab(const FlowSeqWs& w, const AxisTab& x, const AxisTab& y) {
    return FlowResizeTab{w.d_ti + x.i0, w.d_ti + x.i1, w.d_ti + y.i0, w.d_ti + y.i1, w.d_tf + x.w0, w.d_tf + x.w1, w.d_tf + y.w0, w.d_tf + y.w1};
}

int ensure_seq_ws(Ctx* c, int rows, int cols, const rsdsfm_flow_params& p, FlowSeqWs** out) {
    FlowSeqWs* w = seq_ws_of(c);
    *out = w;
    const int B = batch_of(w);
    if (w->d_buf && w->B == B && w->rows == rows && w->cols == cols && w->min_size == p.min_size && w->downscale == p.downscale && w->sigma == p.sigma)
        return RSDSFM_OK;
    if (w->d_buf || w->d_ring) {
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // the previous batch may still read them
        if (w->d_buf) RSDSFM_HIP_CHECK(c, hipFree(w->d_buf));
        if (w->d_ring) RSDSFM_HIP_CHECK(c, hipFree(w->d_ring));
        w->d_buf = w->d_ring = nullptr;
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
    w->stride = Arena::need(4 * (size_t)rows * cols) / 4;  // (256-byte aligned planes)
    w->pstride = Arena::need(4 * total) / 4;
    const size_t pair_planes = 12 + 1 + FLOW_NDERIV + FLOW_NCOEF;  // two sets of six, avg, derivatives, coefficients
    static_assert(FLOW_NCOEF >= 2, "the coefficient block holds the B + 1 frames of the horizontal pass");
    const size_t bytes = Arena::need(4 * w->ti.size()) + Arena::need(4 * w->tf.size()) + 4 * (size_t)(B + 1) * w->pstride +
                         4 * pair_planes * (size_t)B * w->stride;
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
    if (!w->ti.empty()) RSDSFM_HIP_CHECK(c, hipMemcpyAsync(w->d_ti, w->ti.data(), 4 * w->ti.size(), hipMemcpyHostToDevice, c->stream));
    RSDSFM_HIP_CHECK(c, hipMemcpyAsync(w->d_tf, w->tf.data(), 4 * w->tf.size(), hipMemcpyHostToDevice, c->stream));
    RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // the host tables are pageable
    w->B = B, w->rows = rows, w->cols = cols, w->min_size = p.min_size, w->downscale = p.downscale, w->sigma = p.sigma;
    return RSDSFM_OK;
}

// the ring of B fields behind rsdsfm_solve_video_dev's d_flows_or_null = NULL (freed with the workspace)
int ensure_ring(Ctx* c, FlowSeqWs* w) {
    if (w->d_ring) return RSDSFM_OK;
    w->ring_stride = Arena::need(16 * (size_t)w->rows * w->cols);
    RSDSFM_HIP_CHECK(c, hipMalloc(&w->d_ring, (size_t)w->B * w->ring_stride));
    return RSDSFM_OK;
}

#define FLOW_LAUNCH(expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            c->err = std::string("deep flow sequence: ") + #expr + ": " + hipGetErrorString(_e);  \
            return RSDSFM_ERR_HIP;                                                                 \
        }                                                                                          \
    } while (0)

// one batch: frames[0 .. n] -> flows[0 .. n - 1] (n <= w->B), the launches of flow_host.hip's deep_flow_enqueue, each for all n pairs
int batch_enqueue(Ctx* c, const FlowSeqWs* w, const uint8_t* const* frames, int n, int channels, const rsdsfm_flow_params& p, double* const* flows) {
    hipStream_t s = c->stream;
    const int nl = (int)w->lr.size();
    FlowFramePtrs fp{};
    for (int f = 0; f <= n; ++f) fp.p[f] = frames[f];
    FlowOutPtrs op{};
    for (int q = 0; q < n; ++q) op.p[q] = flows[q];
    FLOW_LAUNCH(flow_seq_presmooth(s, fp, n + 1, w->rows, w->cols, channels, w->d_tf, w->radius, w->c[0], w->stride, w->pyr, w->pstride));
    for (int l = 0; l + 1 < nl; ++l)
        FLOW_LAUNCH(flow_seq_pyr_down(s, w->pyr + w->lvl_off[l], w->lc[l], make_tab(*w, w->down_x[l], w->down_y[l]), w->lr[l + 1], w->lc[l + 1],
                                      w->pyr + w->lvl_off[l + 1], w->pstride, n + 1));
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
        FLOW_LAUNCH(flow_seq_level_entry(s, L, w->stride, w->pyr + w->lvl_off[l], w->pstride, r, cc, C, scale, n));
        // the SOR tiling of flow_host.hip (red-black order: the tiling decides no value)
        const bool single = r <= kFlowRegion && cc <= kFlowRegion;
        const int halo = single ? 0 : 2 * kFlowSorBlock, inner = kFlowRegion - 2 * halo;
        const int tiles_x = (cc + inner - 1) / inner, tiles_y = (r + inner - 1) / inner;
        const int per_launch = single ? p.sor_iterations : kFlowSorBlock;
        int cur = 0;
        for (int f = 0; f < p.fixed_point_iterations; ++f) {
            L.du = S[2 + 2 * cur], L.dv = S[3 + 2 * cur];
            FLOW_LAUNCH(flow_seq_coef(s, L, w->stride, r, cc, k, n));
            for (int done = 0; done < p.sor_iterations; done += per_launch) {
                FlowSorArgs a;
                for (int q = 0; q < FLOW_NCOEF; ++q) a.c[q] = w->c[q];
                a.du_in = S[2 + 2 * cur], a.dv_in = S[3 + 2 * cur];
                a.du_out = S[2 + 2 * (1 - cur)], a.dv_out = S[3 + 2 * (1 - cur)];
                a.rows = r, a.cols = cc, a.halo = halo, a.tiles_x = tiles_x;
                a.nit = std::min(per_launch, p.sor_iterations - done);
                a.om = om, a.om1 = om1;
                FLOW_LAUNCH(flow_seq_sor(s, a, w->stride, tiles_x * tiles_y, n));
                cur = 1 - cur;
            }
        }
        cur_prev = cur;
        if (l == 0) {
            L.du = S[2 + 2 * cur], L.dv = S[3 + 2 * cur];
            FLOW_LAUNCH(flow_seq_output(s, L, w->stride, r, cc, op, n));
        }
    }
    return RSDSFM_OK;
}

template <class T>
bool all_set(const T* const* a, int n) {
    if (!a) return false;
    for (int i = 0; i < n; ++i)
        if (!a[i]) return false;
    return true;
}

int check_clip(Ctx* c, int nframes, int rows, int cols, int channels, const rsdsfm_flow_params* pp, rsdsfm_flow_params* p) {
    int rc = check_args(c, rows, cols, channels, pp, p);
    if (rc != RSDSFM_OK) return rc;
    if (nframes < 2) return fail(c, RSDSFM_ERR_INVALID, "deep flow sequence: nframes must be >= 2");
    return RSDSFM_OK;
}

}  // namespace

void flow_seq_release(Ctx* c) {
    FlowSeqWs* w = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_seq_mutex);
        auto it = g_seq.find(c);
        if (it == g_seq.end()) return;
        w = it->second;
        g_seq.erase(it);
    }
    if (w->d_buf) (void)hipFree(w->d_buf);
    if (w->d_ring) (void)hipFree(w->d_ring);
    delete w;
}

}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_deep_flow_seq_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                             const rsdsfm_flow_params* params_or_null, double* const* d_flows) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    rsdsfm_flow_params p;
    int rc = check_clip(c, nframes, rows, cols, channels, params_or_null, &p);
    if (rc != RSDSFM_OK) return rc;
    if (!all_set(d_frames, nframes) || !all_set(d_flows, nframes - 1)) return fail(c, RSDSFM_ERR_INVALID, "deep flow sequence: null device pointer");
    FlowSeqWs* w = nullptr;
    rc = ensure_seq_ws(c, rows, cols, p, &w);
    for (int g0 = 0; rc == RSDSFM_OK && g0 < nframes - 1; g0 += w->B)
        rc = batch_enqueue(c, w, d_frames + g0, std::min(w->B, nframes - 1 - g0), channels, p, d_flows + g0);
    return rc;
}

int rsdsfm_deep_flow_seq(rsdsfm_ctx* ctx, const uint8_t* const* frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                         const rsdsfm_flow_params* params_or_null, double* const* flows) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    rsdsfm_flow_params p;
    int rc = check_clip(c, nframes, rows, cols, channels, params_or_null, &p);
    if (rc != RSDSFM_OK) return rc;
    if (!all_set(frames, nframes) || !all_set(flows, nframes - 1)) return fail(c, RSDSFM_ERR_INVALID, "deep flow sequence: null pointer");
    FlowSeqWs* w = nullptr;
    rc = ensure_seq_ws(c, rows, cols, p, &w);
    if (rc != RSDSFM_OK) return rc;
    const int B = w->B;
    const size_t npix = (size_t)rows * (size_t)cols, img_bytes = npix * (size_t)channels;
    rc = ensure_stage(c, (size_t)(B + 1) * Arena::need(img_bytes) + (size_t)B * Arena::need(16 * npix));
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
        rc = batch_enqueue(c, w, d_img, n, channels, p, d_flow);
        if (rc != RSDSFM_OK) return rc;
        for (int q = 0; q < n; ++q) RSDSFM_HIP_CHECK(c, hipMemcpyAsync(flows[g0 + q], d_flow[q], 16 * npix, hipMemcpyDeviceToHost, c->stream));
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));  // the next batch overwrites the staging buffer
    }
    return RSDSFM_OK;
}

int rsdsfm_set_flow_batch(rsdsfm_ctx* ctx, int32_t pairs) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    if (pairs < 0 || pairs > kFlowSeqMaxPairs) return fail(c, RSDSFM_ERR_INVALID, "flow batch: pairs must be 0 (default) .. 32");
    seq_ws_of(c)->batch = pairs;  // (the workspace follows on its next use)
    return RSDSFM_OK;
}

int rsdsfm_solve_video_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels, double fx,
                           double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                           const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows_or_null, double* const* d_depth_maps,
                           double* const* d_R_or_null, double* const* d_t_or_null, rsdsfm_frame_result* results) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    rsdsfm_flow_params p;
    int rc = check_clip(c, nframes, rows, cols, channels, flow_params_or_null, &p);
    if (rc != RSDSFM_OK) return rc;
    const int np = nframes - 1;
    if (!params || !results) return fail(c, RSDSFM_ERR_INVALID, "solve video: bad arguments");
    if (!all_set(d_frames, nframes) || !all_set(d_depth_maps, np) || (d_flows_or_null && !all_set(d_flows_or_null, np)) ||
        (d_R_or_null && !all_set(d_R_or_null, np)) || (d_t_or_null && !all_set(d_t_or_null, np)))
        return fail(c, RSDSFM_ERR_INVALID, "solve video: null device pointer");
    FlowSeqWs* w = nullptr;
    rc = ensure_seq_ws(c, rows, cols, p, &w);
    if (rc == RSDSFM_OK && !d_flows_or_null) rc = ensure_ring(c, w);
    if (rc != RSDSFM_OK) return rc;
    const int B = w->B;
    double* fl[kFlowSeqMaxPairs];
    rsdsfm_frame_job jobs[kFlowSeqMaxPairs];
    for (int g0 = 0; g0 < np; g0 += B) {
        const int n = std::min(B, np - g0);
        for (int q = 0; q < n; ++q)
            fl[q] = d_flows_or_null ? d_flows_or_null[g0 + q] : reinterpret_cast<double*>(static_cast<char*>(w->d_ring) + (size_t)q * w->ring_stride);
        rc = batch_enqueue(c, w, d_frames + g0, n, channels, p, fl);
        if (rc != RSDSFM_OK) return rc;
        for (int q = 0; q < n; ++q)
            jobs[q] = rsdsfm_frame_job{fl[q], rows, cols, fx, fy, cx, cy, gamma, d_depth_maps[g0 + q], d_R_or_null ? d_R_or_null[g0 + q] : nullptr,
                                       d_t_or_null ? d_t_or_null[g0 + q] : nullptr, seeds ? seeds[g0 + q] : params->seed};
        rc = rsdsfm_solve_frames_dev(ctx, jobs, n, params, results + g0);
        if (rc != RSDSFM_OK) {
            // rsdsfm_solve_frames_dev numbers the pairs of the batch from 0: number them within the clip
            const size_t colon = c->err.find(':');
            if (g0 > 0 && c->err.compare(0, 5, "pair ") == 0 && colon != std::string::npos)
                c->err = "pair " + std::to_string(g0 + std::stoi(c->err.substr(5, colon - 5))) + c->err.substr(colon);
            return rc;
        }
        for (int i = 0; i < g0; ++i) results[i].d_inliers = nullptr, results[i].d_inlier_idx = nullptr, results[i].d_scanline = nullptr;
    }
    return RSDSFM_OK;
}

}  // extern "C"
