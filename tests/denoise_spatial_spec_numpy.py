"""Executable definition of the spatial top-up (include/rsdsfm_denoise_spatial.h): a single-frame, patch-weighted mean of a
pixel's neighbours in its OWN frame, mixed with the pixel in proportion to what the temporal denoise (tests/denoise_spec_numpy.py) did not give
it.  The kernel (csrc/denoise_spatial_kernels.hip) and the host functions (csrc/denoise_spatial_host.hip) reproduce this file bit for bit.

Integers only.  strength h 1 .. 255 (default 12, the temporal default), target 1 .. 255 (default 80 = 16 (1 + 2 * 2): a fully supported pixel's
weight at the temporal default radius), search S 1 .. 3 (default 2).  All three defaults are choices, not measurements.

inputs       image I (rows, cols[, CH]) uint8, CH 1 or 3; mask m, v(p) = m(p) != 0; weight plane n (uint8) or None: n(p) = 16 where v(p)
candidates   q = p + d, d in [-S, S]^2 without 0, q inside the frame, v(p) and v(q)
patch        over the o in {-1, 0, 1}^2 with p + o and q + o inside the frame and both set: D = sum_o sum_c |I_c(p + o) - I_c(q + o)|,
             N = CH #{o} (>= CH: o = 0 counts); w_q = 16 - min(16, (16 D) // (h N)): the temporal formula between two places of one image
sums         Sw = sum_q w_q, s_c = sum_q w_q I_c(q)
top-up       delta = max(0, target - n(p)); B = max(128, Sw) (128 = eight full-weight candidates, all of S = 1: a wider search only adds
             support); W = n(p) B + delta Sw
             v(p) and W > 0:   out_c = (2 (n B I_c(p) + delta s_c) + W) // (2 W)            (round half up)
             v(p) and W == 0:  out_c = I_c(p)                                               (only with n = 0)
             not v(p):         out_c = 0
support      min(255, (2 W + B) // (2 B)) where v(p), else 0
counts       [unset: not v(p), kept: v(p) and delta Sw == 0 (the output is I(p) byte for byte), smoothed: the rest]

Nothing overflows 32 bits: n B I <= 255 * 768 * 255, delta s_c has the same bound, the numerator stays under 2^31 (asserted below).

Not here: search windows beyond 7 x 7, patches other than 3 x 3, a noise-level estimate.
"""
import numpy as np

import denoise_spec_numpy as temporal

W16 = temporal.W
STRENGTH_DEFAULT, STRENGTH_MAX = temporal.STRENGTH_DEFAULT, 255  # choices, not measurements
TARGET_DEFAULT, TARGET_MAX = W16 * (1 + 2 * temporal.RADIUS_DEFAULT), 255
SEARCH_DEFAULT, SEARCH_MAX = 2, 3
B_MIN = 8 * W16


def _shift(a, dy, dx):
    """b(p) = a(p + (dy, dx)), 0 where p + d lies outside the frame"""
    rows, cols = a.shape[:2]
    S = max(abs(dy), abs(dx))
    p = np.pad(a, [(S, S), (S, S)] + [(0, 0)] * (a.ndim - 2))
    return p[S + dy:S + dy + rows, S + dx:S + dx + cols]


def displacements(search):
    return [(dy, dx) for dy in range(-search, search + 1) for dx in range(-search, search + 1) if (dy, dx) != (0, 0)]


def patch_weight(I, v, dy, dx, strength):
    """the weight of the candidate p + (dy, dx) at every p -> (w (rows, cols) int64, D, N); I (rows, cols, CH) int64, v bool"""
    both = v & _shift(v, dy, dx)
    e = np.where(both, np.abs(I - _shift(I, dy, dx)).sum(axis=-1), 0)
    D, N = temporal.box3(e), I.shape[2] * temporal.box3(both.astype(np.int64))
    w = np.where(both, W16 - np.minimum(W16, (W16 * D) // np.maximum(strength * N, 1)), 0)
    return w, D, N


def denoise_spatial(image, mask, weight=None, strength=STRENGTH_DEFAULT, target=TARGET_DEFAULT, search=SEARCH_DEFAULT):
    """-> dict(image, support (rows, cols) uint8, counts [unset, kept, smoothed], sum_w (rows, cols) int64)"""
    assert 1 <= strength <= STRENGTH_MAX and 1 <= target <= TARGET_MAX and 1 <= search <= SEARCH_MAX
    image = np.ascontiguousarray(image, dtype=np.uint8)
    gray = image.ndim == 2
    I = temporal._planes(image).astype(np.int64)
    rows, cols, ch = I.shape
    assert ch in (1, 3)
    v = np.asarray(mask) != 0
    assert v.shape == (rows, cols)
    n = np.where(v, W16, 0).astype(np.int64) if weight is None else np.asarray(weight).astype(np.int64)
    assert n.shape == (rows, cols) and n.min() >= 0 and n.max() <= 255
    sw = np.zeros((rows, cols), dtype=np.int64)
    s = np.zeros((rows, cols, ch), dtype=np.int64)
    for dy, dx in displacements(search):
        w, _, _ = patch_weight(I, v, dy, dx, strength)
        sw += w
        s += w[..., None] * _shift(I, dy, dx)
    delta = np.maximum(0, target - n)
    B = np.maximum(B_MIN, sw)
    Wt = n * B + delta * sw
    num = 2 * ((n * B)[..., None] * I + delta[..., None] * s) + Wt[..., None]
    assert sw.max() <= W16 * ((2 * search + 1) ** 2 - 1) and num.max() < 2 ** 31 and (2 * Wt + B).max() < 2 ** 31
    out = np.where((v & (Wt > 0))[..., None], num // np.maximum(2 * Wt, 1)[..., None], np.where(v[..., None], I, 0))
    assert out.min() >= 0 and out.max() <= 255
    support = np.where(v, np.minimum(255, (2 * Wt + B) // (2 * B)), 0)
    kept = v & (delta * sw == 0)
    counts = [int((~v).sum()), int(kept.sum()), int((v & ~kept).sum())]
    out = out.astype(np.uint8)
    return dict(image=out[..., 0] if gray else out, support=support.astype(np.uint8), counts=counts, sum_w=sw)


def denoise_spatial_brute(image, mask, weight=None, strength=STRENGTH_DEFAULT, target=TARGET_DEFAULT, search=SEARCH_DEFAULT):
    """the same definition as a loop per pixel, candidate and patch offset, written without the vectorised helpers above
    -> (image, support, counts)"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    I = image.reshape(image.shape[0], image.shape[1], -1)
    rows, cols, ch = I.shape
    out, support, counts = np.zeros_like(I), np.zeros((rows, cols), dtype=np.uint8), [0, 0, 0]
    inside = lambda y, x: 0 <= y < rows and 0 <= x < cols
    for y in range(rows):
        for x in range(cols):
            if mask[y, x] == 0:
                counts[0] += 1
                continue
            n = 16 if weight is None else int(weight[y, x])
            sw, s = 0, [0] * ch
            for dy in range(-search, search + 1):
                for dx in range(-search, search + 1):
                    qy, qx = y + dy, x + dx
                    if (dy == 0 and dx == 0) or not inside(qy, qx) or mask[qy, qx] == 0:
                        continue
                    D = cnt = 0
                    for oy in (-1, 0, 1):
                        for ox in (-1, 0, 1):
                            if inside(y + oy, x + ox) and inside(qy + oy, qx + ox) and mask[y + oy, x + ox] != 0 and mask[qy + oy, qx + ox] != 0:
                                cnt += 1
                                D += sum(abs(int(I[y + oy, x + ox, c]) - int(I[qy + oy, qx + ox, c])) for c in range(ch))
                    w = 16 - min(16, (16 * D) // (strength * ch * cnt))
                    sw += w
                    for c in range(ch):
                        s[c] += w * int(I[qy, qx, c])
            delta = max(0, target - n)
            B = max(128, sw)
            Wt = n * B + delta * sw
            for c in range(ch):
                out[y, x, c] = (2 * (n * B * int(I[y, x, c]) + delta * s[c]) + Wt) // (2 * Wt) if Wt > 0 else I[y, x, c]
            support[y, x] = min(255, (2 * Wt + B) // (2 * B))
            counts[1 if delta * sw == 0 else 2] += 1
    return out.reshape(image.shape), support, counts
