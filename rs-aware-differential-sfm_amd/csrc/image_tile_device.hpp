// image_tile_device.hpp -- what the image stages' kernels share on the device (shutter, retime, denoise, super-resolution, clean plate, and the
// packed-byte primitives of the blend, the crop and the inpaint): every function is __device__ __forceinline__, so a kernel built from these
// blocks is the code it was when it carried its own copy.  DESIGN section 12, "Shared tile toolkit and clip walk".
//   packed bytes    a thread owns 4 consecutive pixels; a plane's 4 (mask) or 4 CH (image) bytes travel as dwords, one byte or halfword per field.
//   the tile        a workgroup of kBP threads owns 16 rows x 64 columns, a thread 4 consecutive pixels of one row.  A kernel that needs a pixel's
//                   3 x 3 neighbourhood keeps one packed dword per pixel in LDS, 18 rows x 66 dwords = 4 752 B, the tile's pixel (y, x) at
//                   [y + 1][x + 1]; the halo of 1 about the tile -- 2 * 66 + 2 * 16 = 164 pixels -- is formed by threads 0 .. 163, one each.
//                   A thread reads its 3 x 6 window as nine 8-byte reads at [row][4 g .. 4 g + 5] (8-byte aligned: 66 and 4 g are even; the
//                   compiler pairs them as ds_read2_b64).  For a 64-bit read the bank is (addr / 4) mod 64 and a wave is served as lanes 0 - 31
//                   and 32 - 63: the 16 threads of a row cover 16 distinct pairs of banks (stride 4 dwords), and the next row, 66 dwords on,
//                   lies 2 banks further: the 32 lanes of a group take 32 distinct bank pairs -- no conflict.  (A stride of 64 or 68 would put
//                   the second row on the first row's banks.)  The own pixels' stores are 4 ds_write_b32 per thread, 2-way, which costs a store
//                   nothing.
//   the cells       a pixel's cell is CH + 1 uint16 [sums, n]: BGR cells (8 B, the ABI's alignment) move as 16-byte accesses (8-byte where the
//                   row's tail is shorter than 4), gray cells (4 B) as one 16-byte access where the pixel index is even and the four pixels
//                   are in the row, else per pixel.
//   the outputs     whole dwords where the thread's four pixels are in the row and start on a dword, else byte by byte.
//   the counters    a sum per thread, shuffles, LDS, one 64-bit integer atomicAdd per counter and workgroup: exact and independent of scheduling.
#pragma once

#include <stdint.h>

#include "denoise.hpp"
#include "rectify_dense_device.hpp"

namespace rsdsfm {

// ---------------------------------------------------------------------------------------------------
// packed bytes
// ---------------------------------------------------------------------------------------------------
// 1 in every byte of w that is not 0
__device__ __forceinline__ unsigned bytes_set(unsigned w) { return ((w | ((w & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u; }
__device__ __forceinline__ unsigned bytes_zero(unsigned w) { return bytes_set(w) ^ 0x01010101u; }

// byte k of an array of dwords (k a compile-time constant after unrolling)
__device__ __forceinline__ unsigned byte_of(const unsigned* w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// halfword k of an array of dwords
__device__ __forceinline__ unsigned half_of(const unsigned* w, int k) { return (w[k >> 1] >> (16 * (k & 1))) & 0xffffu; }

__device__ __forceinline__ unsigned absdiff(unsigned a, unsigned b) { return a > b ? a - b : b - a; }

// a layer's byte under the gain G (Q16): G <= 2^18, the byte < 2^8
__device__ __forceinline__ unsigned gained(unsigned G, unsigned l) {
    const unsigned k = (G * l + 32768u) >> 16;
    return k > 255u ? 255u : k;
}

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

// ND dwords of bytes from byte offset `off` (any alignment) of a plane, as ND + 1 aligned dwords shifted into place: the planes are dense (no
// pitch), so a row starts on a dword only when cols % 4 == 0 -- one path for every cols
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

// ---------------------------------------------------------------------------------------------------
// the 16 x 64 tile
// ---------------------------------------------------------------------------------------------------
constexpr int kTileRows = kDenoiseTileRows, kTileCols = kDenoiseTileCols;
constexpr int kTileLdsStride = kTileCols + 2;                      // 66 dwords: see the bank note above
constexpr int kTileHalo = 2 * (kTileCols + 2) + 2 * kTileRows;     // 164
constexpr int kTileLdsWords = (kTileRows + 2) * kTileLdsStride;   // the tile and its halo, a dword per pixel
static_assert(kTileRows * (kTileCols / 4) == kBP, "a thread owns 4 consecutive pixels of a row of the tile");
static_assert(kTileHalo <= kBP && kTileLdsStride % 2 == 0, "one halo pixel per thread; 8-byte aligned rows");

// grid (ceil(cols / 64), ceil(rows / 16)): at most 256 x 1024
inline dim3 tile_grid(int rows, int cols) { return dim3((unsigned)((cols + kTileCols - 1) / kTileCols), (unsigned)((rows + kTileRows - 1) / kTileRows)); }

// a thread's place: row ty and group g of the tile at (y0, x0), its first pixel (y, x) = flat index p0, and nin, how many of its 4 pixels lie
// inside the frame (the first nin)
struct TileThread {
    int tid, ty, g, y0, x0, y, x, nin;
    int64_t p0;
};

__device__ __forceinline__ TileThread tile_thread(int rows, int cols) {
    TileThread t;
    t.tid = (int)threadIdx.x;
    t.ty = t.tid / (kTileCols / 4);
    t.g = t.tid % (kTileCols / 4);
    t.y0 = (int)blockIdx.y * kTileRows;
    t.x0 = (int)blockIdx.x * kTileCols;
    t.y = t.y0 + t.ty;
    t.x = t.x0 + 4 * t.g;
    t.nin = (t.y < rows && t.x < cols) ? (cols - t.x < 4 ? cols - t.x : 4) : 0;
    t.p0 = (int64_t)t.y * cols + t.x;
    return t;
}

// 1 (first_ones) or 0xff (first_bytes) in each of the first nin bytes
__device__ __forceinline__ unsigned first_ones(int nin) { return nin == 4 ? 0x01010101u : nin == 3 ? 0x00010101u : nin == 2 ? 0x00000101u : nin == 1 ? 0x00000001u : 0u; }
__device__ __forceinline__ unsigned first_bytes(int nin) { return nin == 4 ? 0xffffffffu : nin == 3 ? 0x00ffffffu : nin == 2 ? 0x0000ffffu : nin == 1 ? 0x000000ffu : 0u; }

// halo thread tid < kTileHalo: the rows above and below (66 each), the columns left and right (16 each), one pixel per thread: its place
// (ly, lx) in LDS and (hy, hx) in the frame, which may lie outside it
struct TileHalo {
    int ly, lx, hy, hx;
};

__device__ __forceinline__ TileHalo tile_halo(const TileThread& t) {
    TileHalo h;
    if (t.tid < 2 * kTileLdsStride) {
        h.ly = t.tid < kTileLdsStride ? 0 : kTileRows + 1;
        h.lx = t.tid < kTileLdsStride ? t.tid : t.tid - kTileLdsStride;
    } else {
        const int r = t.tid - 2 * kTileLdsStride;
        h.ly = 1 + (r < kTileRows ? r : r - kTileRows);
        h.lx = r < kTileRows ? 0 : kTileCols + 1;
    }
    h.hy = t.y0 + h.ly - 1;
    h.hx = t.x0 + h.lx - 1;
    return h;
}

// the thread's own four dwords in LDS
__device__ __forceinline__ unsigned* tile_own(unsigned* s_tile, const TileThread& t) { return s_tile + (t.ty + 1) * kTileLdsStride + 4 * t.g + 1; }

// the column sums of the thread's 3 x 6 window: three rows of six columns, 8-byte reads.  A field that stays below its width in a sum of 9 does
// not carry (the stages pack a count <= 9 above a sum <= 9 * 765 = 6 885)
__device__ __forceinline__ void tile_sum3x3(const unsigned* s_tile, int ty, int g, unsigned (&col)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) col[i] = 0u;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const Lds8* q = static_cast<const Lds8*>(__builtin_assume_aligned(s_tile + (ty + r) * kTileLdsStride + 4 * g, 8));
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const Lds8 t = q[i];
            col[2 * i] += t[0];
            col[2 * i + 1] += t[1];
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// the cells of a thread's four pixels, 2 (CH + 1) dwords: cell0 the first cell, the first nin are the thread's
// ---------------------------------------------------------------------------------------------------
// the 16 bytes start on the ABI's 8
template <int CH>
__device__ __forceinline__ bool cells_wide(int nin, int64_t p0) {
    return nin == 4 && (CH == 3 || (p0 & 1) == 0);
}

template <int CH>
__device__ __forceinline__ void cells_load(const unsigned short* cell0, int nin, bool wide, unsigned* cw) {
    constexpr int NW = 2 * (CH + 1);
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

template <int CH>
__device__ __forceinline__ void cells_store(unsigned short* cell0, int nin, bool wide, const unsigned* cw) {
    constexpr int NW = 2 * (CH + 1);
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
}

// ---------------------------------------------------------------------------------------------------
// the output group: the thread's four pixels of an image plane (ow: CH dwords) or of a one-byte plane (word)
// ---------------------------------------------------------------------------------------------------
// p0 and CH * p0 bytes are 4-byte aligned and the four pixels are the thread's
__device__ __forceinline__ bool group_whole(int nin, int64_t p0) { return nin == 4 && (p0 & 3) == 0; }

// the image plane and NP one-byte planes (a NULL plane is skipped) under ONE test, so that a kernel's outputs share the branch
template <int CH, int NP>
__device__ __forceinline__ void store_group(unsigned char* __restrict__ out, const unsigned* ow, unsigned char* const (&plane)[NP], const unsigned (&word)[NP], int64_t p0,
                                            int nin) {
    if (group_whole(nin, p0)) {
#pragma unroll
        for (int d = 0; d < CH; ++d) reinterpret_cast<unsigned*>(out + (int64_t)CH * p0)[d] = ow[d];
#pragma unroll
        for (int k = 0; k < NP; ++k)
            if (plane[k]) *reinterpret_cast<unsigned*>(plane[k] + p0) = word[k];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nin) {
#pragma unroll
                for (int c = 0; c < CH; ++c) out[(int64_t)CH * (p0 + j) + c] = (unsigned char)byte_of(ow, CH * j + c);
#pragma unroll
                for (int k = 0; k < NP; ++k)
                    if (plane[k]) plane[k][p0 + j] = (unsigned char)((word[k] >> (8 * j)) & 0xffu);
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// the counters: counts[k] += the workgroup's sum of n[k], k < K; nothing when counts is NULL (uniform).  Every thread of the workgroup calls it
// ---------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void block_counts_add(unsigned (&n)[K], unsigned long long* __restrict__ counts) {
    __shared__ unsigned s_wave[K][kBP / 64];
    if (!counts) return;  // (uniform)
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n[k] += __shfl_down(n[k], off, 64);
        if ((threadIdx.x & 63) == 0) s_wave[k][threadIdx.x / 64] = n[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        unsigned total = 0;
#pragma unroll
        for (int i = 0; i < kBP / 64; ++i) total += s_wave[threadIdx.x][i];
        if (total) atomicAdd(counts + threadIdx.x, (unsigned long long)total);
    }
}

}  // namespace rsdsfm
