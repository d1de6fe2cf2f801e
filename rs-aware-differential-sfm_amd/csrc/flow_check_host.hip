// flow_check_host.hip -- C ABI of the forward-backward flow check (include/rsdsfm_flow_check.h; tests/flow_check_spec_numpy.py is the
// definition, flow_check_kernels.hip the kernel): the check alone, the checked DeepFlow pair, and the checked clip.  The fields come from
// the one DeepFlow driver (flow_host.hip: flow_enqueue); the clip call is rsdsfm_solve_video_dev's batch loop (flow_seq_host.hip:
// solve_video_run) with a hook between a batch's flow and its solve.  No flow kernel and no solve code of its own.
#include <cmath>

#include "../../include/rsdsfm_flow_check.h"
#include "flow_check.hpp"
#include "flow_host.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"

namespace rsdsfm {
namespace {

using namespace flowhost;

// a device buffer that is made again when another size is asked for (whatever the stream still runs on the old one is waited for)
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int grow(Ctx* c, size_t want, bool exact) {
        if (p && (exact ? bytes == want : bytes >= want)) return RSDSFM_OK;
        if (p) {
            RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
            RSDSFM_HIP_CHECK(c, hipFree(p));
        }
        p = nullptr, bytes = 0;
        RSDSFM_HIP_CHECK(c, hipMalloc(&p, want));
        bytes = want;
        return RSDSFM_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr, bytes = 0;
    }
};

// The context's checked-flow workspace, Ctx::flow_check, every part made on first use and again when its size changes:
struct FlowCheckWs {
    DevBuf bwd;     // rsdsfm_deep_flow_checked_dev: the backward field where the caller passes none (16 B per pixel)
    DevBuf ring;    // rsdsfm_solve_video_checked_dev: B backward fields, next to the clip workspace's forward ring
    DevBuf counts;  // its per-pair counters (one int64 per pair of the clip)
};

FlowCheckWs* check_ws(Ctx* c) {
    if (!c->flow_check) c->flow_check = new FlowCheckWs();
    return static_cast<FlowCheckWs*>(c->flow_check);
}

rsdsfm_flow_check_params check_defaults() { return rsdsfm_flow_check_params{0.01, 0.5}; }

int check_params(Ctx* c, const rsdsfm_flow_check_params* pp, rsdsfm_flow_check_params* p) {
    *p = pp ? *pp : check_defaults();
    if (!std::isfinite(p->a1) || !std::isfinite(p->a2) || p->a1 < 0.0 || p->a2 < 0.0)
        return fail(c, RSDSFM_ERR_INVALID, "flow check: a1 and a2 must be finite and >= 0");
    return RSDSFM_OK;
}

// the counters of the n pairs zeroed (they are contiguous where there are several), then the one launch
int enqueue_check(Ctx* c, const FlowCheckPtrs& t, int n, int rows, int cols, const rsdsfm_flow_check_params& k) {
    if (t.count[0]) RSDSFM_HIP_CHECK(c, hipMemsetAsync(t.count[0], 0, sizeof(long long) * (size_t)n, c->stream));
    RSDSFM_HIP_CHECK(c, flow_check_launch(c->stream, t, n, rows, cols, k.a1, k.a2));
    return RSDSFM_OK;
}

}  // namespace

void flow_check_release(Ctx* c) {
    FlowCheckWs* w = static_cast<FlowCheckWs*>(c->flow_check);
    if (!w) return;
    w->bwd.release(), w->ring.release(), w->counts.release();
    delete w;
    c->flow_check = nullptr;
}

}  // namespace rsdsfm

using namespace rsdsfm;
using namespace rsdsfm::flowhost;

extern "C" {

int rsdsfm_flow_check_default_params(rsdsfm_flow_check_params* out) {
    if (!out) return RSDSFM_ERR_INVALID;
    *out = check_defaults();
    return RSDSFM_OK;
}

int rsdsfm_flow_consistency_dev(rsdsfm_ctx* ctx, const double* d_fwd, const double* d_bwd, int32_t rows, int32_t cols,
                                const rsdsfm_flow_check_params* params_or_null, uint8_t* d_mask, double* d_masked_flow_or_null, double* d_resid_or_null,
                                int64_t* d_count_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (rows < 2 || cols < 2 || rows > 16384 || cols > 16384) return fail(c, RSDSFM_ERR_INVALID, "flow check: sides must be in [2, 16384]");
    rsdsfm_flow_check_params k;
    int rc = check_params(c, params_or_null, &k);
    if (rc != RSDSFM_OK) return rc;
    if (!d_fwd || !d_bwd || !d_mask) return fail(c, RSDSFM_ERR_INVALID, "flow check: null device pointer");
    if ((uintptr_t)d_mask & 3u) return fail(c, RSDSFM_ERR_INVALID, "flow check: the mask must be 4-byte aligned");
    // the masked field may be the forward field; no other output is an input or another output
    const void* in[2] = {d_fwd, d_bwd};
    const void* out[4] = {d_mask, d_masked_flow_or_null, d_resid_or_null, d_count_or_null};
    for (int a = 0; a < 4; ++a) {
        if (!out[a]) continue;
        for (int b = 0; b < 2; ++b)
            if (out[a] == in[b] && !(a == 1 && b == 0)) return fail(c, RSDSFM_ERR_INVALID, "flow check: an output is one of the input fields");
        for (int b = a + 1; b < 4; ++b)
            if (out[a] == out[b]) return fail(c, RSDSFM_ERR_INVALID, "flow check: two outputs share a buffer");
    }
    FlowCheckPtrs t{};
    t.fwd[0] = d_fwd, t.bwd[0] = d_bwd, t.mask[0] = d_mask, t.masked[0] = d_masked_flow_or_null, t.resid[0] = d_resid_or_null;
    t.count[0] = reinterpret_cast<long long*>(d_count_or_null);
    return enqueue_check(c, t, 1, rows, cols, k);
}

int rsdsfm_deep_flow_checked_dev(rsdsfm_ctx* ctx, const uint8_t* d_img1, const uint8_t* d_img2, int32_t rows, int32_t cols, int32_t channels,
                                 const rsdsfm_flow_params* flow_params_or_null, const rsdsfm_flow_check_params* check_params_or_null, double* d_flow,
                                 double* d_bwd_or_null, uint8_t* d_mask, int64_t* d_count_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    rsdsfm_flow_params p;
    int rc = check_args(c, rows, cols, channels, flow_params_or_null, &p);
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_flow_check_params k;
    rc = check_params(c, check_params_or_null, &k);
    if (rc != RSDSFM_OK) return rc;
    if (!d_img1 || !d_img2 || !d_flow || !d_mask) return fail(c, RSDSFM_ERR_INVALID, "checked deep flow: null device pointer");
    if ((uintptr_t)d_mask & 3u) return fail(c, RSDSFM_ERR_INVALID, "flow check: the mask must be 4-byte aligned");
    const void* out[4] = {d_flow, d_mask, d_bwd_or_null, d_count_or_null};
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b)
            if (out[a] && out[a] == out[b]) return fail(c, RSDSFM_ERR_INVALID, "checked deep flow: two outputs share a buffer");
    FlowCheckWs* ws = check_ws(c);
    FlowWs* w = flow_ws(c, true);
    rc = ensure_flow_ws(c, w, 1, rows, cols, p);
    if (rc == RSDSFM_OK && !d_bwd_or_null) rc = ws->bwd.grow(c, 16 * (size_t)rows * (size_t)cols, true);
    if (rc != RSDSFM_OK) return rc;
    // two passes on the pair workspace, the second with the frames swapped: rsdsfm_deep_flow_dev's launches, twice
    double* d_bwd = d_bwd_or_null ? d_bwd_or_null : static_cast<double*>(ws->bwd.p);
    const uint8_t* const there[2] = {d_img1, d_img2};
    const uint8_t* const back[2] = {d_img2, d_img1};
    rc = flow_enqueue(c, w, there, 1, channels, p, &d_flow);
    if (rc == RSDSFM_OK) rc = flow_enqueue(c, w, back, 1, channels, p, &d_bwd);
    if (rc != RSDSFM_OK) return rc;
    FlowCheckPtrs t{};
    t.fwd[0] = d_flow, t.bwd[0] = d_bwd, t.mask[0] = d_mask, t.masked[0] = d_flow, t.count[0] = reinterpret_cast<long long*>(d_count_or_null);
    return enqueue_check(c, t, 1, rows, cols, k);
}

int rsdsfm_solve_video_checked_dev(rsdsfm_ctx* ctx, const uint8_t* const* d_frames, int32_t nframes, int32_t rows, int32_t cols, int32_t channels,
                                   double fx, double fy, double cx, double cy, double gamma, const rsdsfm_flow_params* flow_params_or_null,
                                   const rsdsfm_frame_params* params, const uint64_t* seeds, double* const* d_flows_or_null,
                                   double* const* d_depth_maps, double* const* d_R_or_null, double* const* d_t_or_null, rsdsfm_frame_result* results,
                                   const rsdsfm_flow_check_params* check_params_or_null, uint8_t* const* d_masks, double* const* d_bwd_flows_or_null,
                                   int64_t* consistent_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    rsdsfm_flow_check_params k;
    int rc = check_params(c, check_params_or_null, &k);
    if (rc != RSDSFM_OK) return rc;
    rsdsfm_flow_params flow_p;
    rc = check_args(c, rows, cols, channels, flow_params_or_null, &flow_p);  // (solve_video_run's first check: the ring below needs the sides)
    if (rc != RSDSFM_OK) return rc;
    const int np = nframes - 1;
    FlowCheckWs* ws = check_ws(c);
    const size_t ring_stride = Arena::need(16 * (size_t)rows * (size_t)cols);
    if (np >= 1) {  // (solve_video_run refuses a shorter clip, and checks everything else the two calls share)
        if (!all_set(d_masks, np) || (d_bwd_flows_or_null && !all_set(d_bwd_flows_or_null, np)))
            return fail(c, RSDSFM_ERR_INVALID, "solve video: null device pointer");
        for (int i = 0; i < np; ++i)
            if ((uintptr_t)d_masks[i] & 3u) return fail(c, RSDSFM_ERR_INVALID, "flow check: the mask must be 4-byte aligned");
        if (consistent_or_null) rc = ws->counts.grow(c, sizeof(long long) * (size_t)np, false);
        // the backward ring: one field per pair of a batch (the clip workspace's B: rsdsfm_set_flow_batch)
        if (rc == RSDSFM_OK && !d_bwd_flows_or_null) rc = ws->ring.grow(c, (size_t)video_batch_size(c) * ring_stride, true);
        if (rc != RSDSFM_OK) return rc;
    }
    long long* const d_counts = static_cast<long long*>(ws->counts.p);
    const BatchHook check = [&](const FlowWs* w, const rsdsfm_flow_params& p, int g0, int n, double* const* fields) -> int {
        double* bwd[kFlowSeqMaxPairs];
        for (int q = 0; q < n; ++q)
            bwd[q] = d_bwd_flows_or_null ? d_bwd_flows_or_null[g0 + q] : reinterpret_cast<double*>(static_cast<char*>(ws->ring.p) + (size_t)q * ring_stride);
        // the batch's frames through the reversed pointer array: pair q of it is (frame n - q -> frame n - q - 1), the backward field of pair n - 1 - q
        const uint8_t* rev[kFlowSeqMaxPairs + 1];
        double* rev_out[kFlowSeqMaxPairs];
        for (int f = 0; f <= n; ++f) rev[f] = d_frames[g0 + n - f];
        for (int q = 0; q < n; ++q) rev_out[q] = bwd[n - 1 - q];
        int rc2 = flow_enqueue(c, w, rev, n, channels, p, rev_out);
        if (rc2 != RSDSFM_OK) return rc2;
        FlowCheckPtrs t{};
        for (int q = 0; q < n; ++q) {
            t.fwd[q] = fields[q], t.bwd[q] = bwd[q], t.mask[q] = d_masks[g0 + q], t.masked[q] = fields[q];
            t.count[q] = consistent_or_null ? d_counts + g0 + q : nullptr;
        }
        return enqueue_check(c, t, n, rows, cols, k);
    };
    rc = solve_video_run(ctx, d_frames, nframes, rows, cols, channels, fx, fy, cx, cy, gamma, flow_params_or_null, params, seeds, d_flows_or_null,
                         d_depth_maps, d_R_or_null, d_t_or_null, results, nullptr, false, &check);
    if (rc != RSDSFM_OK) return rc;
    if (consistent_or_null) {
        RSDSFM_HIP_CHECK(c, hipMemcpyAsync(consistent_or_null, d_counts, sizeof(long long) * (size_t)np, hipMemcpyDeviceToHost, c->stream));
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    }
    return RSDSFM_OK;
}

}  // extern "C"
