// superres_kernels.hip -- the multi-frame super-resolution on MI355X (gfx950, wave64): include/rsdsfm_superres.h, defined by
// tests/superres_spec_numpy.py and reproduced bit for bit.  Every value goes to memory through ordinary stores and atomicAdd.
//   superres_warp_kernel<CH>    stage C onto a grid finer than the source's (float64, one rounding per operation, -ffp-contract=off): one lane
//                               per group of 4 consecutive fine pixels of a row, grid-stride over the groups.  Per pixel the target as
//                               window_target forms it with the OUTPUT size, the shared fixed point (warp_fixed_point), the two taps ONCE,
//                               and from the same taps the bilinear sample (warp_sample), the nearest source bytes and the proximity
//                               1 + floor(15 (1 - 2 d_x) (1 - 2 d_y)).  Stores: whole dwords (CH per group and plane for bil and near, one
//                               for prox, one for the optional validity plane) where the group has its four pixels and starts on a dword
//                               -- every group when ocols % 4 == 0 --, else byte by byte.  *top == 0 (the 1 x 1 level of stage A: no valid
//                               depth) gives all-zero planes.  Every byte of the outputs is written: no preset.  Stages A and B are the
//                               existing launches on the source grid.
//   superres_accumulate_kernel<CH, FIRST, LAST>
//                               on the 16 x 64 tile of image_tile_device.hpp, on the fine grid (the plane reads, the LDS layout and its bank
//                               argument, the cells, the output group and the counters are described there).  Stage 1: the two proximity
//                               dwords first (a plane's mask is prox != 0); R's CH dwords where some pixel has both set (LAST: where qR has a
//                               byte set), B's only where some pixel has both; e = sum_c |R_c - k(B_c)| and the packed dword (v << 16) | e to
//                               LDS, 0 outside the frame; the halo byte by byte.  Stage 2: the 3 x 3 sum is D in the low half and the count
//                               in the high half; w = 16 - min(16, 16 D / (h CH count)) where v; u = (w qL + 8) >> 4.  Only a thread with
//                               some u != 0 reads the layer's NEAREST plane (CH dwords), only FIRST reads the reference's.  A mid step
//                               whose four u are 0 neither reads nor writes its cells.  FIRST: the cells are not read, cell =
//                               [qR RN_c, qR].  LAST: the cells are not written; out_c = (2 s_c + n) / (2 n) where n > qR, R_c where
//                               n == qR > 0, else 0; mask n > 0; the weight plane n.
//                               A mid step of a BGR frame moves 1 + 1 + 3 + 3 + 3 + 8 + 8 = 27 B per fine pixel where both planes are set
//                               and the weight is not 0.  Gains per workgroup from the 8-word record (seam_gain, threads 0 .. CH - 1,
//                               through LDS): no host wait behind the sums kernel.  The three counters [unset, own only, merged] only in
//                               LAST and only when a counter pointer was passed.
#include <algorithm>

#include "image_tile_device.hpp"
#include "rectify_dense.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_fill.hpp"
#include "stabilize_window_device.hpp"
#include "superres.hpp"

namespace rsdsfm {

namespace {

static_assert(kSuperresProxMax == kDenoiseW, "the own frame's nearest sample counts as the denoise's own frame does");

// ---------------------------------------------------------------------------------------------------
// the render's stage C
// ---------------------------------------------------------------------------------------------------
// one fine pixel at target (tx, ty): b[CH] the bilinear sample, n[CH] the nearest source bytes, returns the proximity; all 0 where not valid
template <int CH>
__device__ __forceinline__ unsigned superres_pixel(const unsigned char* __restrict__ img, const float2* __restrict__ disp, int rows, int cols, int iterations, double tx,
                                                   double ty, unsigned* b, unsigned* n) {
    double px, py;
    const bool valid = warp_fixed_point(disp, rows, cols, iterations, tx, ty, px, py);
    const Tap ax = tap(px, cols), ay = tap(py, rows);  // the taps once: both samples and the proximity come from them
    warp_sample<CH>(img, cols, ax, ay, valid, b);
    const int nx = ax.a < 0.5 ? ax.i0 : ax.i1, ny = ay.a < 0.5 ? ay.i0 : ay.i1;  // the a = 0.5 tie goes to i1
    const unsigned char* s = img + ((int64_t)ny * cols + nx) * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) n[c] = valid ? (unsigned)s[c] : 0u;
    const double ux = 1.0 - ax.a, uy = 1.0 - ay.a;
    const double dx = ax.a < ux ? ax.a : ux, dy = ay.a < uy ? ay.a : uy;
    const double f = 15.0 * ((1.0 - 2.0 * dx) * (1.0 - 2.0 * dy));  // in [0, 15]
    return valid ? 1u + (unsigned)(int)f : 0u;                     // f >= 0: truncation is floor
}

template <int CH>
__device__ __forceinline__ void superres_warp_body(const unsigned char* __restrict__ img, const float2* __restrict__ disp, const double* __restrict__ top, int rows,
                                                   int cols, int orows, int ocols, int iterations, const CropMap wm, unsigned char* __restrict__ bil,
                                                   unsigned char* __restrict__ near, unsigned char* __restrict__ prox, unsigned char* __restrict__ vplane) {
    const bool any = *top != 0.0;  // the 1 x 1 level: 0 = no valid depth = all-zero outputs (uniform)
    const int gpr = (ocols + 3) >> 2;  // groups per row
    const int64_t ngroups = (int64_t)orows * gpr, stride = (int64_t)gridDim.x * kBP;
    for (int64_t g = (int64_t)blockIdx.x * kBP + threadIdx.x; g < ngroups; g += stride) {
        const int Y = (int)(g / gpr), X0 = 4 * (int)(g - (int64_t)Y * gpr);
        const int nin = ocols - X0 < 4 ? ocols - X0 : 4;  // the group's pixels inside the row: 1 .. 4
        const double ty = (wm.r0 + ((double)Y + 0.5) * wm.sy) - 0.5;
        unsigned b[4 * CH], n[4 * CH], q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int c = 0; c < CH; ++c) b[CH * j + c] = n[CH * j + c] = 0u;
            q[j] = 0u;
            if (any && j < nin) {
                const double tx = (wm.c0 + ((double)(X0 + j) + 0.5) * wm.sx) - 0.5;
                q[j] = superres_pixel<CH>(img, disp, rows, cols, iterations, tx, ty, b + CH * j, n + CH * j);
            }
        }
        const int64_t p0 = (int64_t)Y * ocols + X0;
        if (group_whole(nin, p0)) {
            unsigned* db = reinterpret_cast<unsigned*>(bil + (int64_t)CH * p0);
            unsigned* dn = reinterpret_cast<unsigned*>(near + (int64_t)CH * p0);
#pragma unroll
            for (int d = 0; d < CH; ++d) {
                db[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
                dn[d] = n[4 * d] | (n[4 * d + 1] << 8) | (n[4 * d + 2] << 16) | (n[4 * d + 3] << 24);
            }
            const unsigned qw = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            *reinterpret_cast<unsigned*>(prox + p0) = qw;
            if (vplane) *reinterpret_cast<unsigned*>(vplane + p0) = bytes_set(qw);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nin) {
#pragma unroll
                    for (int c = 0; c < CH; ++c) {
                        bil[(int64_t)CH * (p0 + j) + c] = (unsigned char)b[CH * j + c];
                        near[(int64_t)CH * (p0 + j) + c] = (unsigned char)n[CH * j + c];
                    }
                    prox[p0 + j] = (unsigned char)q[j];
                    if (vplane) vplane[p0 + j] = (unsigned char)(q[j] ? 1u : 0u);
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// the accumulate
// ---------------------------------------------------------------------------------------------------
template <int CH, bool FIRST, bool LAST>
__device__ __forceinline__ void superres_accumulate_body(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rnear,
                                                         const unsigned char* __restrict__ rprox, const unsigned char* __restrict__ layer,
                                                         const unsigned char* __restrict__ lnear, const unsigned char* __restrict__ lprox, int rows, int cols,
                                                         const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode, unsigned strength,
                                                         unsigned short* __restrict__ cells, unsigned char* __restrict__ out, unsigned char* __restrict__ mask_out,
                                                         unsigned char* __restrict__ weight, unsigned long long* __restrict__ counts) {
    constexpr int H = CH + 1;      // halfwords per cell
    constexpr int NW = 4 * H / 2;  // dwords of a thread's four cells: 8 (BGR) or 4 (gray)
    __shared__ __attribute__((aligned(16))) unsigned s_tile[kTileLdsWords];
    __shared__ unsigned s_gain[CH];
    const bool has_layer = layer != nullptr;  // (uniform)
    const TileThread t = tile_thread(rows, cols);
    const int nin = t.nin;
    const int64_t p0 = t.p0, npix = (int64_t)rows * cols;
    const unsigned inside = first_bytes(nin);

    unsigned qr = 0u, ql = 0u, v = 0u, rw[CH], u[4] = {0u, 0u, 0u, 0u};  // qr, ql: the four proximities; v: 1 in the bytes with both set
#pragma unroll
    for (int d = 0; d < CH; ++d) rw[d] = 0u;

    if (nin) {  // the proximity dwords first
        unsigned w1[1];
        load_bytes<1>(rprox, p0, npix, w1);
        qr = w1[0] & inside;
        if (has_layer && qr) {
            load_bytes<1>(lprox, p0, npix, w1);
            ql = w1[0] & inside;
            v = bytes_set(qr) & bytes_set(ql);
        }
        if (LAST ? qr != 0u : v != 0u) load_bytes<CH>(ref, (int64_t)CH * p0, (int64_t)CH * npix, rw);  // image bytes under an empty plane are not read
    }

    unsigned G[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) G[c] = kGainOne;
    if (has_layer) {
        if (t.tid < CH) s_gain[t.tid] = sums ? seam_gain(sums, CH, t.tid, min_overlap, gain_mode) : kGainOne;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CH; ++c) G[c] = s_gain[c];
        // stage 1: the thread's own four pixels, on the bilinear samples
        unsigned ent[4] = {0u, 0u, 0u, 0u};
        if (v) {
            unsigned lw[CH];
            load_bytes<CH>(layer, (int64_t)CH * p0, (int64_t)CH * npix, lw);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned e = 0u;
#pragma unroll
                for (int c = 0; c < CH; ++c) e += absdiff(byte_of(rw, CH * j + c), gained(G[c], byte_of(lw, CH * j + c)));
                ent[j] = ((v >> (8 * j)) & 1u) ? (0x10000u | e) : 0u;
            }
        }
        unsigned* row = tile_own(s_tile, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) row[j] = ent[j];
        if (t.tid < kTileHalo) {
            const TileHalo h = tile_halo(t);
            unsigned e = 0u;
            if (h.hy >= 0 && h.hy < rows && h.hx >= 0 && h.hx < cols) {
                const int64_t p = (int64_t)h.hy * cols + h.hx;
                if (rprox[p] != 0 && lprox[p] != 0) {
                    e = 0x10000u;
#pragma unroll
                    for (int c = 0; c < CH; ++c) e += absdiff(ref[CH * p + c], gained(G[c], layer[CH * p + c]));
                }
            }
            s_tile[h.ly * kTileLdsStride + h.lx] = e;
        }
        __syncthreads();
        // stage 2: the 3 x 3 sums of the packed dwords
        if (v) {
            unsigned col[6];
            tile_sum3x3(s_tile, t.ty, t.g, col);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned s = col[j] + col[j + 1] + col[j + 2];
                const unsigned D = s & 0xffffu, cnt = s >> 16;
                if ((v >> (8 * j)) & 1u) {  // the pixel itself counts: cnt >= 1
                    const unsigned qd = (kDenoiseW * D) / (strength * (unsigned)CH * cnt);
                    const unsigned w = kDenoiseW - (qd > kDenoiseW ? kDenoiseW : qd);
                    u[j] = (w * ((ql >> (8 * j)) & 0xffu) + 8u) >> 4;
                }
            }
        }
    }

    unsigned n3[3] = {0u, 0u, 0u};  // [unset, own only, merged]; at most 4 per thread
    const bool any_u = (u[0] | u[1] | u[2] | u[3]) != 0u;
    if (nin && (FIRST || LAST || any_u)) {  // a mid step that adds nothing neither reads nor writes its cells
        unsigned cw[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) cw[i] = 0u;
        const bool wide = cells_wide<CH>(nin, p0);
        unsigned short* cell0 = (FIRST && LAST) ? nullptr : cells + (int64_t)H * p0;
        if (!FIRST) cells_load<CH>(cell0, nin, wide, cw);
        // the nearest samples: the reference's only in FIRST, the layer's only where something is added
        unsigned rn[CH], ln[CH];
#pragma unroll
        for (int d = 0; d < CH; ++d) rn[d] = ln[d] = 0u;
        if (FIRST && qr) load_bytes<CH>(rnear, (int64_t)CH * p0, (int64_t)CH * npix, rn);
        if (any_u) load_bytes<CH>(lnear, (int64_t)CH * p0, (int64_t)CH * npix, ln);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned add[H];
            const unsigned own = FIRST ? ((qr >> (8 * j)) & 0xffu) : 0u;
#pragma unroll
            for (int c = 0; c < CH; ++c) add[c] = own * byte_of(rn, CH * j + c) + u[j] * gained(G[c], byte_of(ln, CH * j + c));
            add[CH] = own + u[j];
#pragma unroll
            for (int h = 0; h < H; ++h) cw[(H * j + h) >> 1] += add[h] << (16 * ((H * j + h) & 1));  // no halfword overflows: n <= 240, sums <= 61 200
        }
        if (!LAST) {
            cells_store<CH>(cell0, nin, wide, cw);
        } else {
            unsigned ow[CH], mw = 0u, nw = 0u;
#pragma unroll
            for (int d = 0; d < CH; ++d) ow[d] = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned n = half_of(cw, H * j + CH), q = (qr >> (8 * j)) & 0xffu;
                const unsigned merged = n > q ? 1u : 0u, own = (n == q && q > 0u) ? 1u : 0u, den = merged ? 2u * n : 1u;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const unsigned val = merged ? (2u * half_of(cw, H * j + c) + n) / den : own ? byte_of(rw, CH * j + c) : 0u;  // round half up; <= 255
                    ow[(CH * j + c) >> 2] |= (val & 0xffu) << (8 * ((CH * j + c) & 3));
                }
                mw |= (n > 0u ? 1u : 0u) << (8 * j);
                nw |= (n & 0xffu) << (8 * j);
                if (j < nin) {
                    n3[0] += 1u - merged - own;
                    n3[1] += own;
                    n3[2] += merged;
                }
            }
            unsigned char* const planes[2] = {mask_out, weight};
            const unsigned words[2] = {mw, nw};
            store_group<CH>(out, ow, planes, words, p0, nin);
        }
    }
    if constexpr (LAST) block_counts_add<3>(n3, counts);
}

}  // namespace

// grid-stride over the groups of 4 fine pixels of a row, block kBP.  rows x cols: the source (img, disp); orows x ocols: the outputs.
// r0 / c0 / sy / sx: the window and the scales h / orows, w / ocols (CropMap).  vplane may be NULL
template <int CH>
__global__ __launch_bounds__(kBP) void superres_warp_kernel(const unsigned char* __restrict__ img, const float2* __restrict__ disp, const double* __restrict__ top,
                                                           int rows, int cols, int orows, int ocols, int iterations, double r0, double c0, double sy, double sx,
                                                           unsigned char* __restrict__ bil, unsigned char* __restrict__ near, unsigned char* __restrict__ prox,
                                                           unsigned char* __restrict__ vplane) {
    superres_warp_body<CH>(img, disp, top, rows, cols, orows, ocols, iterations, CropMap{r0, c0, sy, sx}, bil, near, prox, vplane);
}

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP, on the fine planes.  Not LAST: cells += the layer's weighted nearest bytes (FIRST: cells =
// the reference's proximity times its nearest bytes, then the layer).  LAST: out, mask_out and weight (may be NULL) are written whole;
// counts[0 .. 2] += [unset, own only, merged].  layer == lnear == lprox == NULL: no layer (FIRST and LAST)
template <int CH, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBP) void superres_accumulate_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rnear,
                                                                 const unsigned char* __restrict__ rprox, const unsigned char* __restrict__ layer,
                                                                 const unsigned char* __restrict__ lnear, const unsigned char* __restrict__ lprox, int rows, int cols,
                                                                 const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode, unsigned strength,
                                                                 unsigned short* __restrict__ cells, unsigned char* __restrict__ out,
                                                                 unsigned char* __restrict__ mask_out, unsigned char* __restrict__ weight,
                                                                 unsigned long long* __restrict__ counts) {
    superres_accumulate_body<CH, FIRST, LAST>(ref, rnear, rprox, layer, lnear, lprox, rows, cols, sums, min_overlap, gain_mode, strength, cells, out, mask_out, weight,
                                              counts);
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int superres_render_launch(Ctx* c, const DenseWs& ws, const unsigned char* d_img, int channels, const double* d_depth_cm, const double* d_R, const double* d_t, double fx,
                           double fy, double cx, double cy, int rows, int cols, int mode, int q5_mode, int iterations, const StabPose& vp, int scale, const int32_t window[4],
                           unsigned char* d_bil, unsigned char* d_near, unsigned char* d_prox, unsigned char* d_valid) {
    const double* top = nullptr;
    const int rc = rectify_dense_launch_fill(c, ws, d_depth_cm, rows, cols, &top);
    if (rc != RSDSFM_OK) return rc;
    const DensePlan p = rectify_dense_plan(rows, cols);
    const dim3 tiles((cols + kTX - 1) / kTX, (rows + kTY - 1) / kTY);
    hipLaunchKernelGGL(stabilize_map_kernel, tiles, dim3(kCB), 0, c->stream, d_depth_cm, ws.d_pyr, p.h[0], p.w[0], d_R, d_t, fx, fy, cx, cy, q5_mode == 0 ? fx : fy, rows,
                       cols, mode, vp, ws.d_disp, (double*)nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    const int orows = scale * rows, ocols = scale * cols;  // <= 16384 each
    const int64_t ngroups = (int64_t)orows * ((ocols + 3) / 4);
    const int64_t nb = (ngroups + kBP - 1) / kBP;
    const double sy = (double)window[2] / (double)orows, sx = (double)window[3] / (double)ocols;
    hipLaunchKernelGGL(channels == 3 ? superres_warp_kernel<3> : superres_warp_kernel<1>, dim3((unsigned)std::min<int64_t>(nb, 65536)), dim3(kBP), 0, c->stream, d_img,
                       ws.d_disp, top, rows, cols, orows, ocols, iterations, (double)window[0], (double)window[1], sy, sx, d_bil, d_near, d_prox, d_valid);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

int superres_accumulate_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rnear, const unsigned char* d_rprox, const unsigned char* d_layer,
                               const unsigned char* d_lnear, const unsigned char* d_lprox, int channels, int rows, int cols, const unsigned long long* d_sums,
                               int64_t min_overlap, int gain_mode, int strength, uint16_t* d_cells, bool first, bool last, unsigned char* d_image_out,
                               unsigned char* d_mask_out, unsigned char* d_weight, int64_t* d_counts3) {
    if (last && d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    using Kernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, int, int,
                            const unsigned long long*, long long, int, unsigned, unsigned short*, unsigned char*, unsigned char*, unsigned char*, unsigned long long*);
    static const Kernel kernels[2][2][2] = {
        {{superres_accumulate_kernel<1, false, false>, superres_accumulate_kernel<1, false, true>},
         {superres_accumulate_kernel<1, true, false>, superres_accumulate_kernel<1, true, true>}},
        {{superres_accumulate_kernel<3, false, false>, superres_accumulate_kernel<3, false, true>},
         {superres_accumulate_kernel<3, true, false>, superres_accumulate_kernel<3, true, true>}}};
    // the outputs are passed only to the instances that write them
    hipLaunchKernelGGL(kernels[channels == 3][first][last], tile_grid(rows, cols), dim3(kBP), 0, c->stream, d_ref, d_rnear, d_rprox, d_layer, d_lnear, d_lprox, rows, cols, d_sums,
                       (long long)min_overlap, gain_mode, (unsigned)strength, d_cells, last ? d_image_out : nullptr, last ? d_mask_out : nullptr,
                       last ? d_weight : nullptr, last ? reinterpret_cast<unsigned long long*>(d_counts3) : nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
