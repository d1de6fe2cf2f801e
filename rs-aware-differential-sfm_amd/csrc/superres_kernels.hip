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
//                               denoise_accumulate_kernel's 2-D tile (denoise_kernels.hip) on the fine grid: a workgroup of kBP threads owns
//                               16 rows x 64 columns, a thread 4 consecutive pixels of one row; planes read as ALIGNED dwords of the flat
//                               array shifted into place (one path for every cols).  Stage 1: the two proximity dwords first (a plane's
//                               mask is prox != 0); R's CH dwords where some pixel has both set (LAST: where qR has a byte set), B's only
//                               where some pixel has both; e = sum_c |R_c - k(B_c)| and the packed dword (v << 16) | e to LDS, 0 outside the
//                               frame; the halo of 1 (164 pixels) by threads 0 .. 163, byte by byte.  LDS: 18 rows x 66 dwords = 4 752 B,
//                               the denoise's layout and bank reasoning (8-byte reads at [row][4 g .. 4 g + 5]; rows 66 dwords apart lie 2
//                               banks apart).  Stage 2: the 3 x 3 sum is D in the low half and the count in the high half;
//                               w = 16 - min(16, 16 D / (h CH count)) where v; u = (w qL + 8) >> 4.  Only a thread with some u != 0 reads
//                               the layer's NEAREST plane (CH dwords), only FIRST reads the reference's.  Cells as the shutter's: BGR cells
//                               (8 B) move as 16-byte accesses (8-byte where the row's tail is shorter than 4), gray cells (4 B) as one
//                               16-byte access where the pixel index is even and the four pixels are in the row, else 4-byte.  A mid step
//                               whose four u are 0 neither reads nor writes its cells.  FIRST: the cells are not read, cell =
//                               [qR RN_c, qR].  LAST: the cells are not written; out_c = (2 s_c + n) / (2 n) where n > qR, R_c where
//                               n == qR > 0, else 0; mask n > 0; the weight plane n.
//                               A mid step of a BGR frame moves 1 + 1 + 3 + 3 + 3 + 8 + 8 = 27 B per fine pixel where both planes are set
//                               and the weight is not 0.  Gains per workgroup from the 8-word record (seam_gain, threads 0 .. CH - 1,
//                               through LDS): no host wait behind the sums kernel.  The three counters [unset, own only, merged]: a sum
//                               per thread, shuffles, LDS, one 64-bit integer atomicAdd each per workgroup, only in LAST and only when a
//                               counter pointer was passed.
#include <algorithm>

#include "rectify_dense.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"
#include "stabilize_fill.hpp"
#include "stabilize_window_device.hpp"
#include "superres.hpp"

namespace rsdsfm {

namespace {

constexpr int kTR = kDenoiseTileRows, kTC = kDenoiseTileCols;
constexpr int kLdsStride = kTC + 2;             // 66 dwords: rows 2 banks apart, 8-byte aligned
constexpr int kHalo = 2 * (kTC + 2) + 2 * kTR;  // 164
static_assert(kTR * (kTC / 4) == kBP, "a thread owns 4 consecutive pixels of a row of the tile");
static_assert(kHalo <= kBP && kLdsStride % 2 == 0, "one halo pixel per thread; 8-byte aligned rows");
static_assert(kSuperresProxMax == kDenoiseW, "the own frame's nearest sample counts as the denoise's own frame does");

// 1 in every byte of w that is not 0
__device__ __forceinline__ unsigned bytes_set(unsigned w) { return ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u; }

// byte k of an array of dwords (k a compile-time constant after unrolling)
__device__ __forceinline__ unsigned byte_of(const unsigned* w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// halfword k of an array of dwords
__device__ __forceinline__ unsigned half_of(const unsigned* w, int k) { return (w[k >> 1] >> (16 * (k & 1))) & 0xffffu; }

// 16 bytes of cells; the ABI promises 8-byte alignment
typedef unsigned Cells16 __attribute__((ext_vector_type(4), aligned(8)));
typedef unsigned Cells8 __attribute__((ext_vector_type(2), aligned(8)));
typedef unsigned Lds8 __attribute__((ext_vector_type(2), aligned(8)));  // one ds_read_b64

// the aligned dword at byte offset o (a multiple of 4) of a plane of nbytes bytes; bytes past the plane's end read as 0 and are not touched
__device__ __forceinline__ unsigned aligned_dword(const unsigned char* __restrict__ base, int64_t o, int64_t nbytes) {
    if (o + 4 <= nbytes) return *reinterpret_cast<const unsigned*>(base + o);
    unsigned w = 0u;
    for (int b = 0; b < 4; ++b)
        if (o + b < nbytes) w |= (unsigned)base[o + b] << (8 * b);
    return w;
}

// ND dwords of bytes from byte offset `off` (any alignment) of a plane, as ND + 1 aligned dwords shifted into place
template <int ND>
__device__ __forceinline__ void load_bytes(const unsigned char* __restrict__ base, int64_t off, int64_t nbytes, unsigned* out) {
    const int64_t a = off & ~(int64_t)3;
    const unsigned sh = 8u * (unsigned)(off & 3);
    unsigned w[ND + 1];
#pragma unroll
    for (int d = 0; d < ND; ++d) w[d] = aligned_dword(base, a + 4 * d, nbytes);
    w[ND] = sh ? aligned_dword(base, a + 4 * ND, nbytes) : 0u;
#pragma unroll
    for (int d = 0; d < ND; ++d) out[d] = sh ? (w[d] >> sh) | (w[d + 1] << (32u - sh)) : w[d];
}

__device__ __forceinline__ unsigned gained(unsigned G, unsigned l) {  // G <= 2^18, the byte < 2^8
    const unsigned k = (G * l + 32768u) >> 16;
    return k > 255u ? 255u : k;
}

__device__ __forceinline__ unsigned absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

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
        if (nin == 4 && (p0 & 3) == 0) {  // p0 and CH * p0 bytes are 4-byte aligned
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
    __shared__ __attribute__((aligned(16))) unsigned s_tile[(kTR + 2) * kLdsStride];
    __shared__ unsigned s_gain[CH];
    const bool has_layer = layer != nullptr;  // (uniform)
    const int tid = (int)threadIdx.x, ty = tid / (kTC / 4), g = tid % (kTC / 4);
    const int y0 = (int)blockIdx.y * kTR, x0 = (int)blockIdx.x * kTC;
    const int y = y0 + ty, x = x0 + 4 * g;
    const int64_t npix = (int64_t)rows * cols;
    const int nin = (y < rows && x < cols) ? (cols - x < 4 ? cols - x : 4) : 0;  // the thread's pixels inside the frame: the first nin of its 4
    const int64_t p0 = (int64_t)y * cols + x;
    const unsigned inside = nin == 4 ? 0xffffffffu : nin == 3 ? 0x00ffffffu : nin == 2 ? 0x0000ffffu : nin == 1 ? 0x000000ffu : 0u;

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
        if (tid < CH) s_gain[tid] = sums ? seam_gain(sums, CH, tid, min_overlap, gain_mode) : kGainOne;
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
        unsigned* row = s_tile + (ty + 1) * kLdsStride + 4 * g + 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) row[j] = ent[j];
        // the halo: the rows above and below (66 each), the columns left and right (16 each), one pixel per thread
        if (tid < kHalo) {
            int ly, lx;
            if (tid < 2 * kLdsStride) {
                ly = tid < kLdsStride ? 0 : kTR + 1;
                lx = tid < kLdsStride ? tid : tid - kLdsStride;
            } else {
                const int r = tid - 2 * kLdsStride;
                ly = 1 + (r < kTR ? r : r - kTR);
                lx = r < kTR ? 0 : kTC + 1;
            }
            const int hy = y0 + ly - 1, hx = x0 + lx - 1;
            unsigned e = 0u;
            if (hy >= 0 && hy < rows && hx >= 0 && hx < cols) {
                const int64_t p = (int64_t)hy * cols + hx;
                if (rprox[p] != 0 && lprox[p] != 0) {
                    e = 0x10000u;
#pragma unroll
                    for (int c = 0; c < CH; ++c) e += absdiff(ref[CH * p + c], gained(G[c], layer[CH * p + c]));
                }
            }
            s_tile[ly * kLdsStride + lx] = e;
        }
        __syncthreads();
        // stage 2: the 3 x 3 sums of the packed dwords; three rows of six columns, 8-byte reads
        if (v) {
            unsigned col[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const Lds8* q = static_cast<const Lds8*>(__builtin_assume_aligned(s_tile + (ty + r) * kLdsStride + 4 * g, 8));
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const Lds8 t = q[i];
                    col[2 * i] += t[0];  // the high half is a count <= 9, the low half <= 6 885: no carry
                    col[2 * i + 1] += t[1];
                }
            }
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
        // the thread's cells: BGR 8 B each (two 16-byte accesses when the four pixels are its own); gray 4 B each
        const bool wide = nin == 4 && (CH == 3 || (p0 & 1) == 0);  // the 16 bytes start on the ABI's 8
        unsigned short* cell0 = (FIRST && LAST) ? nullptr : cells + (int64_t)H * p0;
        if (!FIRST) {
            if (wide) {
#pragma unroll
                for (int k = 0; k < NW / 4; ++k) {
                    const Cells16 t = reinterpret_cast<const Cells16*>(cell0)[k];
#pragma unroll
                    for (int i = 0; i < 4; ++i) cw[4 * k + i] = t[i];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nin) {
                        if constexpr (CH == 3) {
                            const Cells8 t = reinterpret_cast<const Cells8*>(cell0)[j];
                            cw[2 * j] = t[0];
                            cw[2 * j + 1] = t[1];
                        } else {
                            cw[j] = reinterpret_cast<const unsigned*>(cell0)[j];
                        }
                    }
            }
        }
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
            if (wide) {
#pragma unroll
                for (int k = 0; k < NW / 4; ++k) reinterpret_cast<Cells16*>(cell0)[k] = Cells16{cw[4 * k], cw[4 * k + 1], cw[4 * k + 2], cw[4 * k + 3]};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nin) {
                        if constexpr (CH == 3) {
                            reinterpret_cast<Cells8*>(cell0)[j] = Cells8{cw[2 * j], cw[2 * j + 1]};
                        } else {
                            reinterpret_cast<unsigned*>(cell0)[j] = cw[j];
                        }
                    }
            }
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
            if (nin == 4 && (p0 & 3) == 0) {  // p0 and CH * p0 bytes are 4-byte aligned
#pragma unroll
                for (int d = 0; d < CH; ++d) reinterpret_cast<unsigned*>(out + (int64_t)CH * p0)[d] = ow[d];
                *reinterpret_cast<unsigned*>(mask_out + p0) = mw;
                if (weight) *reinterpret_cast<unsigned*>(weight + p0) = nw;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nin) {
#pragma unroll
                        for (int c = 0; c < CH; ++c) out[(int64_t)CH * (p0 + j) + c] = (unsigned char)byte_of(ow, CH * j + c);
                        mask_out[p0 + j] = (unsigned char)((mw >> (8 * j)) & 0xffu);
                        if (weight) weight[p0 + j] = (unsigned char)((nw >> (8 * j)) & 0xffu);
                    }
            }
        }
    }
    if constexpr (LAST) {
        __shared__ unsigned s_wave[3][kBP / 64];
        if (!counts) return;  // (uniform)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) n3[k] += __shfl_down(n3[k], off, 64);
            if ((threadIdx.x & 63) == 0) s_wave[k][threadIdx.x / 64] = n3[k];
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            unsigned total = 0;
#pragma unroll
            for (int i = 0; i < kBP / 64; ++i) total += s_wave[threadIdx.x][i];
            if (total) atomicAdd(counts + threadIdx.x, (unsigned long long)total);
        }
    }
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
    const dim3 grid((unsigned)((cols + kTC - 1) / kTC), (unsigned)((rows + kTR - 1) / kTR));  // at most 256 x 1024
    using Kernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, int, int,
                            const unsigned long long*, long long, int, unsigned, unsigned short*, unsigned char*, unsigned char*, unsigned char*, unsigned long long*);
    static const Kernel kernels[2][2][2] = {
        {{superres_accumulate_kernel<1, false, false>, superres_accumulate_kernel<1, false, true>},
         {superres_accumulate_kernel<1, true, false>, superres_accumulate_kernel<1, true, true>}},
        {{superres_accumulate_kernel<3, false, false>, superres_accumulate_kernel<3, false, true>},
         {superres_accumulate_kernel<3, true, false>, superres_accumulate_kernel<3, true, true>}}};
    // the outputs are passed only to the instances that write them
    hipLaunchKernelGGL(kernels[channels == 3][first][last], grid, dim3(kBP), 0, c->stream, d_ref, d_rnear, d_rprox, d_layer, d_lnear, d_lprox, rows, cols, d_sums,
                       (long long)min_overlap, gain_mode, (unsigned)strength, d_cells, last ? d_image_out : nullptr, last ? d_mask_out : nullptr,
                       last ? d_weight : nullptr, last ? reinterpret_cast<unsigned long long*>(d_counts3) : nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
