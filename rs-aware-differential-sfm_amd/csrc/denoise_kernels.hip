// denoise_kernels.hip -- the temporal denoise's accumulate on MI355X (gfx950, wave64): include/rsdsfm_denoise.h, defined by
// tests/denoise_spec_numpy.py and reproduced bit for bit.  Integer arithmetic only; every value goes to memory through ordinary stores and atomicAdd.
//   denoise_accumulate_kernel<CH, FIRST, LAST>  the image stages' first 2-D tile: a workgroup of kBP threads owns 16 rows x 64 columns, a thread 4
//                               consecutive pixels of one row.  The planes are dense (no pitch), so a row starts on a dword only when
//                               cols % 4 == 0: every plane is read as ALIGNED dwords of the flat array about the thread's bytes and shifted
//                               into place (one path for every cols; a dword that would reach past the plane's end is read byte by byte).
//                               Stage 1: the two mask dwords first; R's CH dwords only where some pixel has both masks set (FIRST: where mR
//                                 has a byte set), L's only where some pixel has both; per pixel k_c = min(255, (G_c L_c + 32768) >> 16),
//                                 e = sum_c |R_c - k_c| and the packed dword (v << 16) | e goes to LDS, 0 for a pixel outside the frame.  The
//                                 halo of 1 about the tile -- 2 * 66 + 2 * 16 = 164 pixels -- is formed by threads 0 .. 163, byte by byte,
//                                 masks first.  Each |R - k| is formed once per workgroup (the halo: once more by the neighbouring workgroup).
//                               LDS: 18 rows x 66 dwords = 4 752 B, the tile's pixel (y, x) at [y + 1][x + 1].  Stage 2 reads a thread's
//                                 3 x 6 window as nine 8-byte reads at [row][4 g .. 4 g + 5] (8-byte aligned: 66 and 4 g are even; the compiler pairs
//                                 them as ds_read2_b64).  For a
//                                 64-bit read the bank is (addr / 4) mod 64 and a wave is served as lanes 0 - 31 and 32 - 63: the 16 threads
//                                 of a row cover 16 distinct pairs of banks (stride 4 dwords), and the next row, 66 dwords on, lies 2 banks
//                                 further: the 32 lanes of a group take 32 distinct bank pairs -- no conflict.  (A stride of 64 or 68 would
//                                 put the second row on the first row's banks.)  Stage 1's stores are 4 ds_write_b32 per thread, 2-way, which
//                                 costs a store nothing.
//                               Stage 2: the sum of the 3 x 3 packed dwords is D in the low half (<= 9 * 765 = 6 885) and the count in the high
//                                 half; w = 16 - min(16, 16 D / (h CH count)) where v, else 0.  The cells as the shutter's: CH + 1 uint16 per
//                                 pixel; BGR cells (8 B, the ABI's alignment) move as 16-byte accesses, gray cells (4 B) as one 16-byte access
//                                 where the pixel index is even and its four pixels are in the row, else per pixel.  A mid step
//                                 (neither FIRST nor LAST) whose four weights are 0 neither reads nor writes its cells.  FIRST: the cells are
//                                 not read.  LAST: the cells are not written; out_c = (2 s_c + n) / (2 n) and mask 1 where n > 0, else 0 / 0,
//                                 the weight plane n; whole dwords where the four pixels start on one, else byte by byte: every byte of the
//                                 outputs is written, no preset.
//                               A mid step of a BGR frame moves 3 + 1 + 3 + 1 + 8 + 8 = 24 B per pixel where both masks are set, plus the halo's
//                                 164 / 1024 of the first 8.
//                               Every workgroup computes the CH gains itself from the 8-word record (seam_gain, threads 0 .. CH - 1, through
//                               LDS): no host wait behind the sums kernel.  The three counters [unset, own only, averaged] as the shutter's: a
//                               sum per thread, shuffles, LDS, one 64-bit integer atomicAdd each per workgroup, only in LAST and only when
//                               a counter pointer was passed.
#include <algorithm>

#include "denoise.hpp"
#include "rectify_dense_device.hpp"
#include "rsdsfm_internal.hpp"

namespace rsdsfm {

namespace {

constexpr int kTR = kDenoiseTileRows, kTC = kDenoiseTileCols;
constexpr int kLdsStride = kTC + 2;                 // 66 dwords: see the bank note above
constexpr int kHalo = 2 * (kTC + 2) + 2 * kTR;      // 164
static_assert(kTR * (kTC / 4) == kBP, "a thread owns 4 consecutive pixels of a row of the tile");
static_assert(kHalo <= kBP && kLdsStride % 2 == 0, "one halo pixel per thread; 8-byte aligned rows");

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

template <int CH, bool FIRST, bool LAST>
__device__ __forceinline__ void denoise_accumulate_body(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                        const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                        const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode, unsigned strength,
                                                        unsigned short* __restrict__ cells, unsigned char* __restrict__ out, unsigned char* __restrict__ mask_out,
                                                        unsigned char* __restrict__ weight, unsigned long long* __restrict__ counts) {
    constexpr int H = CH + 1;     // halfwords per cell
    constexpr int NW = 4 * H / 2; // dwords of a thread's four cells: 8 (BGR) or 4 (gray)
    __shared__ __attribute__((aligned(16))) unsigned s_tile[(kTR + 2) * kLdsStride];
    __shared__ unsigned s_gain[CH];
    const bool has_layer = layer != nullptr;  // (uniform)
    const int tid = (int)threadIdx.x, ty = tid / (kTC / 4), g = tid % (kTC / 4);
    const int y0 = (int)blockIdx.y * kTR, x0 = (int)blockIdx.x * kTC;
    const int y = y0 + ty, x = x0 + 4 * g;
    const int64_t npix = (int64_t)rows * cols;
    const int nin = (y < rows && x < cols) ? (cols - x < 4 ? cols - x : 4) : 0;  // the thread's pixels inside the frame: the first nin of its 4
    const int64_t p0 = (int64_t)y * cols + x;
    const unsigned inside = nin == 4 ? 0x01010101u : nin == 3 ? 0x00010101u : nin == 2 ? 0x00000101u : nin == 1 ? 0x00000001u : 0u;

    unsigned mr = 0u, v = 0u, rw[CH], kk[4][CH], wgt[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int d = 0; d < CH; ++d) rw[d] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < CH; ++c) kk[j][c] = 0u;

    if (nin) {  // the mask dwords first
        unsigned w1[1];
        load_bytes<1>(rmask, p0, npix, w1);
        mr = bytes_set(w1[0]) & inside;
        if (has_layer && mr) {
            load_bytes<1>(lmask, p0, npix, w1);
            v = bytes_set(w1[0]) & mr;
        }
        if (FIRST ? mr != 0u : v != 0u) load_bytes<CH>(ref, (int64_t)CH * p0, (int64_t)CH * npix, rw);  // image bytes under an empty mask are not read
    }

    if (has_layer) {
        if (tid < CH) s_gain[tid] = sums ? seam_gain(sums, CH, tid, min_overlap, gain_mode) : kGainOne;
        __syncthreads();
        unsigned G[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) G[c] = s_gain[c];
        // stage 1: the thread's own four pixels
        unsigned ent[4] = {0u, 0u, 0u, 0u};
        if (v) {
            unsigned lw[CH];
            load_bytes<CH>(layer, (int64_t)CH * p0, (int64_t)CH * npix, lw);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned e = 0u;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    kk[j][c] = gained(G[c], byte_of(lw, CH * j + c));
                    e += absdiff(byte_of(rw, CH * j + c), kk[j][c]);
                }
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
                if (rmask[p] != 0 && lmask[p] != 0) {
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
                    wgt[j] = kDenoiseW - (qd > kDenoiseW ? kDenoiseW : qd);
                }
            }
        }
    }

    unsigned n3[3] = {0u, 0u, 0u};  // [unset, own only, averaged]; at most 4 per thread
    const bool any_w = (wgt[0] | wgt[1] | wgt[2] | wgt[3]) != 0u;
    if (nin && (FIRST || LAST || any_w)) {  // a mid step that adds nothing neither reads nor writes its cells
        unsigned cw[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) cw[i] = 0u;
        // the thread's cells: BGR 8 B each (always two 16-byte accesses when the four pixels are its own); gray 4 B each
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
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned add[H];
            const unsigned own = FIRST ? ((mr >> (8 * j)) & 1u) * kDenoiseW : 0u;
#pragma unroll
            for (int c = 0; c < CH; ++c) add[c] = own * byte_of(rw, CH * j + c) + wgt[j] * kk[j][c];
            add[CH] = own + wgt[j];
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
                const unsigned n = half_of(cw, H * j + CH);
                const unsigned ok = n > 0u ? 1u : 0u, den = ok ? 2u * n : 1u;
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const unsigned val = ok ? (2u * half_of(cw, H * j + c) + n) / den : 0u;  // round half up; <= 255
                    ow[(CH * j + c) >> 2] |= val << (8 * ((CH * j + c) & 3));
                }
                mw |= ok << (8 * j);
                nw |= (n & 0xffu) << (8 * j);
                if (j < nin) {
                    n3[0] += 1u - ok;
                    n3[1] += n == kDenoiseW ? 1u : 0u;
                    n3[2] += n > kDenoiseW ? 1u : 0u;
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

// grid (ceil(cols / 64), ceil(rows / 16)), block kBP.  Not LAST: cells += the layer's weighted bytes (FIRST: cells = 16 x the reference, then the
// layer).  LAST: out, mask_out and weight (may be NULL) are written whole; counts[0 .. 2] += [unset, own only, averaged].  layer == lmask ==
// NULL: no layer (FIRST and LAST)
template <int CH, bool FIRST, bool LAST>
__global__ __launch_bounds__(kBP) void denoise_accumulate_kernel(const unsigned char* __restrict__ ref, const unsigned char* __restrict__ rmask,
                                                                const unsigned char* __restrict__ layer, const unsigned char* __restrict__ lmask, int rows, int cols,
                                                                const unsigned long long* __restrict__ sums, long long min_overlap, int gain_mode, unsigned strength,
                                                                unsigned short* __restrict__ cells, unsigned char* __restrict__ out,
                                                                unsigned char* __restrict__ mask_out, unsigned char* __restrict__ weight,
                                                                unsigned long long* __restrict__ counts) {
    denoise_accumulate_body<CH, FIRST, LAST>(ref, rmask, layer, lmask, rows, cols, sums, min_overlap, gain_mode, strength, cells, out, mask_out, weight, counts);
}

// ---------------------------------------------------------------------------------------------------
// launcher
// ---------------------------------------------------------------------------------------------------
int denoise_accumulate_launch(Ctx* c, const unsigned char* d_ref, const unsigned char* d_rmask, const unsigned char* d_layer, const unsigned char* d_lmask, int channels,
                              int rows, int cols, const unsigned long long* d_sums, int64_t min_overlap, int gain_mode, int strength, uint16_t* d_cells, bool first,
                              bool last, unsigned char* d_image_out, unsigned char* d_mask_out, unsigned char* d_weight, int64_t* d_counts3) {
    if (last && d_counts3) RSDSFM_HIP_CHECK(c, hipMemsetAsync(d_counts3, 0, 3 * sizeof(int64_t), c->stream));
    const dim3 grid((unsigned)((cols + kTC - 1) / kTC), (unsigned)((rows + kTR - 1) / kTR));  // at most 256 x 1024
    using Kernel = void (*)(const unsigned char*, const unsigned char*, const unsigned char*, const unsigned char*, int, int, const unsigned long long*, long long, int,
                            unsigned, unsigned short*, unsigned char*, unsigned char*, unsigned char*, unsigned long long*);
    static const Kernel kernels[2][2][2] = {
        {{denoise_accumulate_kernel<1, false, false>, denoise_accumulate_kernel<1, false, true>},
         {denoise_accumulate_kernel<1, true, false>, denoise_accumulate_kernel<1, true, true>}},
        {{denoise_accumulate_kernel<3, false, false>, denoise_accumulate_kernel<3, false, true>},
         {denoise_accumulate_kernel<3, true, false>, denoise_accumulate_kernel<3, true, true>}}};
    // the outputs are passed only to the instances that write them
    hipLaunchKernelGGL(kernels[channels == 3][first][last], grid, dim3(kBP), 0, c->stream, d_ref, d_rmask, d_layer, d_lmask, rows, cols, d_sums, (long long)min_overlap,
                       gain_mode, (unsigned)strength, d_cells, last ? d_image_out : nullptr, last ? d_mask_out : nullptr, last ? d_weight : nullptr,
                       last ? reinterpret_cast<unsigned long long*>(d_counts3) : nullptr);
    RSDSFM_HIP_CHECK(c, hipGetLastError());
    return RSDSFM_OK;
}

}  // namespace rsdsfm
