// fuse_host.hip -- C ABI of the fusion of a clip's depth maps (include/rsdsfm_fuse.h; tests/fuse_spec_numpy.py is the definition,
// fuse_kernels.hip the kernels).  Pairs run in chunks of kLinkMax: for the pairs [a, b) of a chunk the planes of the links a - 1 .. b - 2 are
// preset to all ones, ONE launch splats them and ONE launch merges the chunk's pairs.  Nothing waits on the host between the launches.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/rsdsfm_fuse.h"
#include "fuse.hpp"
#include "rsdsfm_internal.hpp"
#include "sequence_host.hpp"

namespace rsdsfm {
namespace {

// The context's fusion workspace, Ctx::fuse, made on first use and grown when more is asked for:
struct FuseWs {
    void* planes = nullptr;  // splat planes of the links in flight: 8 B per pixel per link
    size_t plane_bytes = 0;
    unsigned long long* counters = nullptr;  // kFuseCounters words per pair of the call
    size_t counter_pairs = 0;
};

int fuse_grow(Ctx* c, void** buf, size_t* have, size_t want, size_t bytes) {
    if (*have >= want) return RSDSFM_OK;
    if (*buf) {
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        RSDSFM_HIP_CHECK(c, hipFree(*buf));
    }
    *buf = nullptr, *have = 0;
    RSDSFM_HIP_CHECK(c, hipMalloc(buf, bytes));
    *have = want;
    return RSDSFM_OK;
}

int fuse_ws(Ctx* c, size_t plane_bytes, size_t pairs, FuseWs** out) {
    if (!c->fuse) c->fuse = new FuseWs();
    FuseWs* w = static_cast<FuseWs*>(c->fuse);
    int rc = fuse_grow(c, &w->planes, &w->plane_bytes, plane_bytes, plane_bytes);
    if (rc != RSDSFM_OK) return rc;
    rc = fuse_grow(c, reinterpret_cast<void**>(&w->counters), &w->counter_pairs, pairs, sizeof(unsigned long long) * kFuseCounters * pairs);
    if (rc != RSDSFM_OK) return rc;
    *out = w;
    return RSDSFM_OK;
}

rsdsfm_fuse_params fuse_defaults() { return rsdsfm_fuse_params{0.1, (int32_t)sizeof(rsdsfm_fuse_params), 0}; }

bool usable(const rsdsfm_link_record& r) { return r.valid && std::isfinite(r.ratio) && r.ratio > 0.0; }  // rsdsfm_chain_clip's rule

int fuse_run(Ctx* c, const double* const* d_fields, const double* const* d_maps, const double* v, const double* w, const double* k, int npairs, int rows,
             int cols, const LinkCamera& cam, double tol, const rsdsfm_link_record* records, double* const* d_fused, uint8_t* const* d_flags,
             uint64_t* const* d_planes, rsdsfm_fuse_record* out_records) {
    const int nlinks = npairs - 1;
    const size_t plane_stride = Arena::need(8 * (size_t)rows * (size_t)cols);
    FuseWs* ws = nullptr;
    int rc = fuse_ws(c, d_planes ? 0 : (size_t)std::min(nlinks, kLinkMax) * plane_stride, (size_t)npairs, &ws);
    if (rc != RSDSFM_OK) return rc;
    RSDSFM_HIP_CHECK(c, hipMemsetAsync(ws->counters, 0, sizeof(unsigned long long) * kFuseCounters * (size_t)npairs, c->stream));
    for (int a = 0; a < npairs; a += kLinkMax) {
        const int b = std::min(npairs, a + kLinkMax);
        const int lo = std::max(a - 1, 0), nl = (b - 2) - lo + 1;  // the chunk's links lo .. b - 2 (none for a single pair)
        auto plane_of = [&](int q) {
            return d_planes ? reinterpret_cast<unsigned long long*>(d_planes[q])
                            : reinterpret_cast<unsigned long long*>(static_cast<char*>(ws->planes) + (size_t)(q - lo) * plane_stride);
        };
        if (nl > 0) {
            FuseSplatArgs s{};
            if (!d_planes) RSDSFM_HIP_CHECK(c, hipMemsetAsync(ws->planes, 0xFF, (size_t)nl * plane_stride, c->stream));
            for (int l = 0; l < nl; ++l) {
                const int q = lo + l;
                if (d_planes) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_planes[q], 0xFF, 8 * (size_t)rows * (size_t)cols, c->stream));
                s.field[l] = d_fields[q], s.z[l] = d_maps[q], s.plane[l] = plane_of(q);
                s.v2[l] = v[3 * q + 2], s.w0[l] = w[3 * q], s.w1[l] = w[3 * q + 1], s.k[l] = k[q];
                s.ratio[l] = usable(records[q]) ? records[q].ratio : 0.0;
            }
            RSDSFM_HIP_CHECK(c, fuse_splat_launch(c->stream, s, cam, nl, rows, cols));
        }
        FuseMergeArgs m{};
        for (int l = 0; l < b - a; ++l) {
            const int p = a + l;
            const bool has_prev = p >= 1 && usable(records[p - 1]), has_next = p + 1 < npairs && usable(records[p]);
            m.field[l] = has_next ? d_fields[p] : nullptr, m.z[l] = d_maps[p], m.zn[l] = has_next ? d_maps[p + 1] : nullptr;
            m.plane[l] = has_prev ? plane_of(p - 1) : nullptr;
            m.fused[l] = d_fused[p], m.flags[l] = d_flags ? d_flags[p] : nullptr;
            m.v2[l] = v[3 * p + 2], m.w0[l] = w[3 * p], m.w1[l] = w[3 * p + 1], m.k[l] = k[p];
            m.ratio[l] = has_next ? records[p].ratio : 0.0;
        }
        RSDSFM_HIP_CHECK(c, fuse_merge_launch(c->stream, m, cam, b - a, rows, cols, tol, ws->counters + (size_t)a * kFuseCounters));
    }
    if (out_records) {
        std::vector<unsigned long long> host((size_t)npairs * kFuseCounters);
        RSDSFM_HIP_CHECK(c, hipMemcpyAsync(host.data(), ws->counters, sizeof(unsigned long long) * host.size(), hipMemcpyDeviceToHost, c->stream));
        RSDSFM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        for (int p = 0; p < npairs; ++p) {
            const unsigned long long* h = host.data() + (size_t)p * kFuseCounters;
            out_records[p] = rsdsfm_fuse_record{(int64_t)h[0], (int64_t)h[1], (int64_t)h[2], (int64_t)h[3], (int64_t)h[4], (int64_t)h[5]};
        }
    }
    return RSDSFM_OK;
}

}  // namespace

void fuse_release(Ctx* c) {
    FuseWs* w = static_cast<FuseWs*>(c->fuse);
    if (!w) return;
    if (w->planes) (void)hipFree(w->planes);
    if (w->counters) (void)hipFree(w->counters);
    delete w;
    c->fuse = nullptr;
}

}  // namespace rsdsfm

using namespace rsdsfm;

extern "C" {

int rsdsfm_fuse_params_init(rsdsfm_fuse_params* params) {
    if (!params) return RSDSFM_ERR_INVALID;
    *params = fuse_defaults();
    return RSDSFM_OK;
}

int rsdsfm_fuse_depths_dev(rsdsfm_ctx* ctx, const double* const* d_fields, const double* const* d_depth_maps, const double* v_3n, const double* w_3n,
                           const double* k_n, int32_t npairs, int32_t rows, int32_t cols, double fx, double fy, double cx, double cy, double gamma,
                           int32_t global_shutter, const rsdsfm_link_record* records, const rsdsfm_fuse_params* params_or_null,
                           double* const* d_fused_maps, uint8_t* const* d_flags_or_null, uint64_t* const* d_splat_planes_or_null,
                           rsdsfm_fuse_record* out_records_or_null) {
    if (!ctx) return RSDSFM_ERR_INVALID;
    Ctx* c = &ctx->c;
    DeviceGuard device_guard_(c);
    if (npairs < 1) return fail(c, RSDSFM_ERR_INVALID, "fuse: npairs must be >= 1");
    if (rows < 2 || cols < 2 || rows > 16384 || cols > 16384) return fail(c, RSDSFM_ERR_INVALID, "fuse: sides must be in [2, 16384]");
    if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.0 || fy == 0.0 || !std::isfinite(gamma) || gamma <= 0.0)
        return fail(c, RSDSFM_ERR_INVALID, "fuse: fx, fy must be finite and non-zero, gamma finite and > 0");
    const rsdsfm_fuse_params p = params_or_null ? *params_or_null : fuse_defaults();
    if (p.struct_bytes != 0 && p.struct_bytes != (int32_t)sizeof(rsdsfm_fuse_params))
        return fail(c, RSDSFM_ERR_INVALID, "rsdsfm_fuse_params: struct_bytes is neither 0 nor sizeof(rsdsfm_fuse_params) -- caller built against another header (use rsdsfm_fuse_params_init)");
    if (!std::isfinite(p.tol) || p.tol < 0.0) return fail(c, RSDSFM_ERR_INVALID, "fuse: tol must be finite and >= 0");
    if (!v_3n || !w_3n || !k_n || (npairs > 1 && !records)) return fail(c, RSDSFM_ERR_INVALID, "fuse: null pointer");
    const int nl = npairs - 1;
    if ((nl > 0 && !all_set(d_fields, nl)) || !all_set(d_depth_maps, npairs) || !all_set(d_fused_maps, npairs) ||
        (d_flags_or_null && !all_set(d_flags_or_null, npairs)) || (nl > 0 && d_splat_planes_or_null && !all_set(d_splat_planes_or_null, nl)))
        return fail(c, RSDSFM_ERR_INVALID, "fuse: null device pointer");
    // every output against every input and every other output
    std::vector<const void*> in, out;
    for (int q = 0; q < npairs; ++q) {
        in.push_back(d_depth_maps[q]);
        if (q < nl) in.push_back(d_fields[q]);
        out.push_back(d_fused_maps[q]);
        if (d_flags_or_null) out.push_back(d_flags_or_null[q]);
        if (q < nl && d_splat_planes_or_null) out.push_back(d_splat_planes_or_null[q]);
    }
    for (size_t a = 0; a < out.size(); ++a) {
        if (std::find(in.begin(), in.end(), out[a]) != in.end()) return fail(c, RSDSFM_ERR_INVALID, "fuse: an output is an input (the pairs are fused from the original maps)");
        if (std::find(out.begin() + a + 1, out.end(), out[a]) != out.end()) return fail(c, RSDSFM_ERR_INVALID, "fuse: two outputs share a buffer");
    }
    const LinkCamera cam{fx, fy, cx, cy, gamma, global_shutter ? 1 : 0};
    return fuse_run(c, d_fields, d_depth_maps, v_3n, w_3n, k_n, npairs, rows, cols, cam, p.tol, records, d_fused_maps, d_flags_or_null,
                    nl > 0 ? d_splat_planes_or_null : nullptr, out_records_or_null);
}

}  // extern "C"
