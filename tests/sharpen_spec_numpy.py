"""Executable definition of the sharpen stage (include/rsdsfm_sharpen.h): a noise-gated unsharp mask.  Every image stage behind the solve
leaves its frame softer than its source (bilinear sampling, box-sensor merges, averaging denoisers); this stage restores local contrast at the
end of the chain without amplifying the noise the noise curve measured and without ringing at edges.  The kernel
(csrc/sharpen_kernels.hip) and the host functions (csrc/sharpen_host.hip) reproduce this file bit for bit.  tests/noise_curve_spec_numpy.py
is imported unchanged: the strength table and a pixel's level are its.

Integers only.

inputs       image I (rows, cols[, 3]) uint8, mask m, v(p) = m(p) != 0; amount_q4 0 .. 64 (16 = 1.0), coring_q4 0 .. 64, overshoot 0 .. 255;
             the strength h: one number 1 .. 255, or lut[level of p] from the 256-entry table of noise_curve_spec_numpy.strengths
blur         k = [1, 4, 6, 4, 1], k(o) = k[oy + 2] k[ox + 2] for o in [-2, 2]^2.  Over the o with p + o inside the frame and v(p + o):
             S_c(p) = sum k(o) I_c(p + o), K(p) = sum k(o).  K <= 256; where v(p), K >= 36
detail       d_c = K I_c(p) - S_c: scaled by K, nothing is divided yet
threshold    the level of p is its byte (gray) or (b + g + r + 1) // 3 (BGR); T = (coring_q4 h + 8) >> 4, the same for every channel
coring       soft: e_c = max(0, |d_c| - T K)
gain         r_c = (2 amount_q4 e_c + 16 K) // (32 K): the magnitude rounded half up; o_c = I_c(p) + sign(d_c) r_c
limit        lo_c, hi_c = the minimum and maximum of I_c over the set pixels of the 3 x 3 block about p inside the frame, p included;
             out_c = clamp(o_c, max(0, lo_c - overshoot), min(255, hi_c + overshoot))
outputs      out where v(p), 0 in every channel where not; the mask is the input's and is not written
counters     [unset, kept, sharpened, limited], exclusive, summing to rows cols: unset: not v(p); kept: out == I in every channel; limited:
             not kept and the limit changed o_c in some channel; sharpened: the rest
bounds       |d_c| <= 255 (K - 36) < 65 280; T may reach 1020, but from T = 255 on e_c = 0 (|d_c| < 255 K), so a kernel may clamp T to 255 and then
             T K <= 255 * 256; 2 * 64 * e + 16 K < 2^24: everything fits 32 bits

The defaults (amount_q4 = 16, coring_q4 = 8, overshoot = 0, strength 12) are choices, not measurements.  0 is a meaningful value of the first
three (the identity, no coring, no overshoot), so they have no "0: the default".

Not here: deconvolution with an estimated point-spread function, radii other than the 5 x 5 binomial, a gain per brightness band, sharpening
inside the super-resolution's accumulate.
"""
import numpy as np

import noise_curve_spec_numpy as curve_spec

AMOUNT_DEFAULT, CORING_DEFAULT, OVERSHOOT_DEFAULT, STRENGTH_DEFAULT = 16, 8, 0, 12
AMOUNT_MAX, CORING_MAX, OVERSHOOT_MAX, STRENGTH_MAX = 64, 64, 255, 255
K1 = (1, 4, 6, 4, 1)


def _planes(image):
    image = np.asarray(image)
    return image[..., None] if image.ndim == 2 else image


def _shift(a, dy, dx, fill=0):
    """b(p) = a(p + (dy, dx)) where that lies inside the frame, else fill"""
    rows, cols = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, rows), slice(0, rows - dy)) if dy >= 0 else (slice(0, rows + dy), slice(-dy, rows))
    xs, xd = (slice(dx, cols), slice(0, cols - dx)) if dx >= 0 else (slice(0, cols + dx), slice(-dx, cols))
    b[yd, xd] = a[ys, xs]
    return b


def blur_sums(image, mask):
    """-> (S (rows, cols, CH) int64, K (rows, cols) int64)"""
    I = _planes(image).astype(np.int64)
    v = (np.asarray(mask) != 0).astype(np.int64)
    Iv = I * v[..., None]
    S, K = np.zeros_like(I), np.zeros_like(v)
    for oy in range(-2, 3):
        for ox in range(-2, 3):
            k = K1[oy + 2] * K1[ox + 2]
            S += k * _shift(Iv, oy, ox)
            K += k * _shift(v, oy, ox)
    return S, K


def local_range(image, mask):
    """-> (lo, hi) (rows, cols, CH) int64 over the set pixels of the 3 x 3 block; lo = 255, hi = 0 where the block holds none"""
    I = _planes(image).astype(np.int64)
    v = (np.asarray(mask) != 0)[..., None]
    lo_in, hi_in = np.where(v, I, 255), np.where(v, I, 0)
    lo, hi = np.full_like(I, 255), np.zeros_like(I)
    for oy in range(-1, 2):
        for ox in range(-1, 2):
            lo = np.minimum(lo, _shift(lo_in, oy, ox, 255))
            hi = np.maximum(hi, _shift(hi_in, oy, ox, 0))
    return lo, hi


def sharpen(image, mask=None, amount_q4=AMOUNT_DEFAULT, coring_q4=CORING_DEFAULT, overshoot=OVERSHOOT_DEFAULT, strength=STRENGTH_DEFAULT, lut=None):
    """-> dict(image, counts [unset, kept, sharpened, limited]).  lut (256,): the strength per pixel, in `strength`'s place"""
    assert 0 <= amount_q4 <= AMOUNT_MAX and 0 <= coring_q4 <= CORING_MAX and 0 <= overshoot <= OVERSHOOT_MAX and 1 <= strength <= STRENGTH_MAX
    image = np.ascontiguousarray(image, dtype=np.uint8)
    gray = image.ndim == 2
    I = _planes(image).astype(np.int64)
    rows, cols, _ = I.shape
    mask = np.full((rows, cols), 255, dtype=np.uint8) if mask is None else np.asarray(mask)
    v = mask != 0
    S, K = blur_sums(image, mask)
    assert K.max() <= 256 and (not v.any() or K[v].min() >= 36)
    K3 = K[..., None]
    d = K3 * I - S
    h = np.full((rows, cols), int(strength), dtype=np.int64) if lut is None else np.asarray(lut).astype(np.int64)[curve_spec.pixel_levels(image)]
    T = (coring_q4 * h + 8) >> 4
    e = np.maximum(0, np.abs(d) - (T * K)[..., None])
    num = 2 * amount_q4 * e + 16 * K3
    assert np.abs(d)[v].max(initial=0) <= 65280 and (np.minimum(T, 255) * K).max() <= 255 * 256 and num.max() < 2 ** 24
    r = num // np.maximum(32 * K3, 1)
    o = I + np.sign(d) * r
    lo, hi = local_range(image, mask)
    out = np.clip(o, np.maximum(0, lo - overshoot), np.minimum(255, hi + overshoot))
    v3 = v[..., None]
    out = np.where(v3, out, 0)
    kept = v & (out == I).all(axis=-1)
    limited = v & ~kept & (out != o).any(axis=-1)
    counts = [int((~v).sum()), int(kept.sum()), int((v & ~kept & ~limited).sum()), int(limited.sum())]
    assert sum(counts) == rows * cols
    out = out.astype(np.uint8)
    return dict(image=out[..., 0] if gray else out, counts=counts)


def sharpen_frame(image, mask=None, amount_q4=AMOUNT_DEFAULT, coring_q4=CORING_DEFAULT, overshoot=OVERSHOOT_DEFAULT, strength=STRENGTH_DEFAULT, quantile_q8=0, scale=0,
                  min_samples=0, band_min_samples=0):
    """the frame's own noise curve measured, then sharpen at its strength per pixel; `strength` is the fallback
    -> dict(image, counts, curve (9, 4) uint64, lut (256,) uint8)"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    mask = np.full(image.shape[:2], 255, dtype=np.uint8) if mask is None else np.asarray(mask)
    curve = curve_spec.noise_curve(image, mask, quantile_q8)["curve"]
    lut = curve_spec.strengths(curve, scale, strength, min_samples, band_min_samples)
    return dict(sharpen(image, mask, amount_q4, coring_q4, overshoot, strength, lut), curve=curve, lut=lut)
