"""Executable definition of the noise curve (include/rsdsfm_noise_curve.h): one frame's noise measured PER BRIGHTNESS LEVEL, and the denoise
strength h(L) that follows from it per pixel.  A sensor's noise is signal-dependent (sigma^2 roughly a L + b), so the single h of
tests/noise_spec_numpy.py is too wide in the shadows and too narrow in the highlights of one and the same frame.  The kernels
(csrc/noise_curve_kernels.hip) and host functions (csrc/noise_curve_host.hip) reproduce this file bit for bit.  tests/noise_spec_numpy.py,
tests/denoise_spec_numpy.py and tests/denoise_spatial_spec_numpy.py are imported unchanged; only what differs is restated.

Integers only.

samples      the candidates, the samples and r = sum K I_c exactly as noise_spec_numpy.responses
level        of the sample (p, c): S = the sum of channel c's nine bytes about p, L = (S + 4) // 9, in 1 .. 254 (a sample's bytes are)
band         b = L >> 5: eight bands of 32 levels
histogram    hist[b][min(|r|, 1023)] += 1: 8 x 1024 uint32; the bands sum to noise_spec_numpy.histogram exactly
curve        36 uint64, nine rows [n, m, sigma_q8, 0]: rows 0 .. 7 noise_spec_numpy.resolve of each band's histogram, row 8 the same of their
             sum, which is noise_spec_numpy.noise_level's record
strengths    256 bytes h(L).  Row 8 with n < min_samples (0: 1024): every entry is the fallback.  Band b is valid iff n_b >= band_min_samples
             (0: 256; a choice, not a measurement).  mfill_b = m_b for a valid band, else the m of the nearest valid band (the lower one on a
             tie), row 8's m when no band is valid.  Centres c_b = 32 b + 16.  L < 16: M32 = 32 mfill_0; L >= 240: M32 = 32 mfill_7; else
             b = (L - 16) >> 5, t = (L - 16) & 31, M32 = (32 - t) mfill_b + t mfill_{b + 1} (linear between centres: no band border shows).
             h(L) = clamp((scale M32 + 256) >> 9, 1, 255).  With every mfill equal to m this is noise_strength's (scale m + 8) >> 4.
consumers    a pixel's level is its byte (gray) or (b + g + r + 1) // 3 (BGR).  The temporal accumulate takes the level of the REFERENCE pixel
             R(p), the top-up the level of the centre pixel p; the weight formulas are the existing ones with `strength` replaced by h(level).

Not here: a sigma per channel, a fitted a L + b model in place of eight medians, monotonicity enforcement, the super-resolution and the
sharpness transfer.
"""
import numpy as np

import denoise_spatial_spec_numpy as spatial
import denoise_spec_numpy as temporal
import noise_spec_numpy as noise

BANDS, BAND_SHIFT = 8, 5
BINS = noise.BINS
BAND_MIN_SAMPLES_DEFAULT = 256  # a choice, not a measurement
W = temporal.W


# ---------------------------------------------------------------------------------------------------
# the measurement
# ---------------------------------------------------------------------------------------------------
def levels(image):
    """-> L (rows - 2, cols - 2, CH) int64: (S + 4) // 9 about every interior pixel, per channel"""
    I = noise._planes(image).astype(np.int64)
    rows, cols, _ = I.shape
    S = np.zeros((rows - 2, cols - 2, I.shape[2]), dtype=np.int64)
    for dy in range(3):
        for dx in range(3):
            S += I[dy:dy + rows - 2, dx:dx + cols - 2]
    return (S + 4) // 9


def histogram(image, mask):
    """-> hist (8, 1024) uint32"""
    r, sample = noise.responses(image, mask)
    L = levels(image)[sample]
    assert L.size == 0 or (L.min() >= 1 and L.max() <= 254)
    key = ((L >> BAND_SHIFT) << 10) | np.minimum(np.abs(r[sample]), BINS - 1)
    return np.bincount(key, minlength=BANDS * BINS).astype(np.uint32).reshape(BANDS, BINS)


def resolve(hist, quantile_q8=0):
    """-> curve (9, 4) uint64"""
    hist = np.asarray(hist).reshape(BANDS, BINS)
    rows = [noise.resolve(hist[b], quantile_q8) for b in range(BANDS)]
    rows.append(noise.resolve(hist.astype(np.uint64).sum(axis=0), quantile_q8))
    return np.array(rows, dtype=np.uint64)


def noise_curve(image, mask, quantile_q8=0):
    """-> dict(hist (8, 1024) uint32, curve (9, 4) uint64)"""
    hist = histogram(image, mask)
    return dict(hist=hist, curve=resolve(hist, quantile_q8))


# ---------------------------------------------------------------------------------------------------
# the strength table
# ---------------------------------------------------------------------------------------------------
def mfill(curve, band_min_samples=0):
    """-> eight Python ints"""
    curve = np.asarray(curve, dtype=np.uint64).reshape(9, 4)
    bms = int(band_min_samples) or BAND_MIN_SAMPLES_DEFAULT
    assert bms >= 0
    valid = [int(curve[b, 0]) >= bms for b in range(BANDS)]
    out = []
    for b in range(BANDS):
        pick = None
        for d in range(BANDS):  # the nearest valid band, the lower one on a tie
            for j in (b - d, b + d):
                if pick is None and 0 <= j < BANDS and valid[j]:
                    pick = j
        out.append(int(curve[8, 1]) if pick is None else int(curve[pick, 1]))
    return out


def strengths(curve, scale=0, fallback=12, min_samples=0, band_min_samples=0):
    """-> lut (256,) uint8: h(L)"""
    curve = np.asarray(curve, dtype=np.uint64).reshape(9, 4)
    scale, min_samples = int(scale) or noise.SCALE_DEFAULT, int(min_samples) or noise.MIN_SAMPLES_DEFAULT
    assert 1 <= scale <= noise.SCALE_MAX and min_samples >= 0 and 1 <= fallback <= noise.STRENGTH_MAX
    if int(curve[8, 0]) < min_samples:
        return np.full(256, fallback, dtype=np.uint8)
    mf = mfill(curve, band_min_samples)
    lut = np.zeros(256, dtype=np.uint8)
    for L in range(256):
        if L < 16:
            M32 = 32 * mf[0]
        elif L >= 240:
            M32 = 32 * mf[7]
        else:
            b, t = (L - 16) >> 5, (L - 16) & 31
            M32 = (32 - t) * mf[b] + t * mf[b + 1]
        lut[L] = min(max((scale * M32 + 256) >> 9, 1), 255)
    return lut


# ---------------------------------------------------------------------------------------------------
# the consumers
# ---------------------------------------------------------------------------------------------------
def pixel_levels(image):
    """-> (rows, cols) int64: the byte (gray) or (b + g + r + 1) // 3 (BGR)"""
    I = noise._planes(image).astype(np.int64)
    return I[..., 0] if I.shape[2] == 1 else (I.sum(axis=-1) + 1) // 3


def weights(ref, ref_mask, layer, layer_mask, G, lut):
    """denoise_spec_numpy.weights with strength = lut[level of R(p)] -> (w, k)"""
    R = temporal._planes(ref).astype(np.int64)
    k = temporal.gained(layer, G)
    v = (np.asarray(ref_mask) != 0) & (np.asarray(layer_mask) != 0)
    e = np.where(v, np.abs(R - k).sum(axis=-1), 0)
    D, N = temporal.box3(e), R.shape[2] * temporal.box3(v.astype(np.int64))
    h = np.asarray(lut).astype(np.int64)[pixel_levels(ref)]
    w = np.where(v, W - np.minimum(W, (W * D) // np.maximum(h * N, 1)), 0)
    return w, k


def step(cells, ref, ref_mask, layer, layer_mask, first, lut, record=None, min_overlap=temporal.MIN_OVERLAP_DEFAULT, gain_mode=0):
    """denoise_spec_numpy.step with the weights above"""
    if layer is None:
        return temporal.step(cells, ref, ref_mask, None, None, first)
    R = temporal._planes(ref).astype(np.int64)
    base = temporal.step(cells, ref, ref_mask, None, None, first).astype(np.int64)
    w, k = weights(ref, ref_mask, layer, layer_mask, temporal.gains(record, R.shape[2], min_overlap, gain_mode), lut)
    total = base + np.concatenate([w[..., None] * k, w[..., None]], axis=-1)
    assert total[..., -1].max() <= W * (1 + temporal.LAYERS_MAX) and total.max() <= 255 * W * (1 + temporal.LAYERS_MAX)
    return total.astype(np.uint16)


def denoise(ref, ref_mask, layers, lut, records=None, min_overlap=temporal.MIN_OVERLAP_DEFAULT, gain_mode=0):
    """denoise_spec_numpy.denoise with the strength per pixel -> resolve's dict plus cells"""
    steps = list(layers) if layers else [(None, None)]
    cells, trail = None, []
    for j, (image, mask) in enumerate(steps):
        cells = step(cells, ref, ref_mask, image, mask, j == 0, lut, records[j] if records is not None and layers else None, min_overlap, gain_mode)
        trail.append(cells)
    return dict(temporal.resolve(cells, np.asarray(ref).ndim == 2), cells=trail)


def denoise_spatial(image, mask, lut, weight=None, target=spatial.TARGET_DEFAULT, search=spatial.SEARCH_DEFAULT):
    """denoise_spatial_spec_numpy.denoise_spatial with strength = lut[level of p] -> dict(image, support, counts)"""
    assert 1 <= target <= spatial.TARGET_MAX and 1 <= search <= spatial.SEARCH_MAX
    image = np.ascontiguousarray(image, dtype=np.uint8)
    gray = image.ndim == 2
    I = temporal._planes(image).astype(np.int64)
    rows, cols, ch = I.shape
    v = np.asarray(mask) != 0
    n = np.where(v, W, 0).astype(np.int64) if weight is None else np.asarray(weight).astype(np.int64)
    h = np.asarray(lut).astype(np.int64)[pixel_levels(image)]
    sw = np.zeros((rows, cols), dtype=np.int64)
    s = np.zeros((rows, cols, ch), dtype=np.int64)
    for dy, dx in spatial.displacements(search):
        w, _, _ = spatial.patch_weight(I, v, dy, dx, h)
        sw += w
        s += w[..., None] * spatial._shift(I, dy, dx)
    delta = np.maximum(0, target - n)
    B = np.maximum(spatial.B_MIN, sw)
    Wt = n * B + delta * sw
    num = 2 * ((n * B)[..., None] * I + delta[..., None] * s) + Wt[..., None]
    assert num.max() < 2 ** 31 and (2 * Wt + B).max() < 2 ** 31
    out = np.where((v & (Wt > 0))[..., None], num // np.maximum(2 * Wt, 1)[..., None], np.where(v[..., None], I, 0)).astype(np.uint8)
    support = np.where(v, np.minimum(255, (2 * Wt + B) // (2 * B)), 0)
    kept = v & (delta * sw == 0)
    counts = [int((~v).sum()), int(kept.sum()), int((v & ~kept).sum())]
    return dict(image=out[..., 0] if gray else out, support=support.astype(np.uint8), counts=counts)
