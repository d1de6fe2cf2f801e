"""Executable definition of the noise level (include/rsdsfm_noise.h): one frame's noise, measured from the frame itself, and the denoise strength
h that follows from it.  The reference has no counterpart (main.cc:380-523 solves pairs one by one and never looks at a frame's noise); this file
is the definition and the kernels (csrc/noise_kernels.hip) and host functions (csrc/noise_host.hip) reproduce it bit for bit.

Integers only.

mask K       [[1, -2, 1], [-2, 4, -2], [1, -2, 1]]: Immerkaer's noise mask, the difference of two discrete Laplacians.  It annihilates constant,
             linear and xy terms of the image, so what it answers on a smooth image is noise.  sum K^2 = 36: on i.i.d. noise of standard
             deviation sigma the response r has standard deviation 6 sigma.
candidates   pixel p with 1 <= y <= rows - 2 and 1 <= x <= cols - 2 whose nine mask bytes (its 3 x 3 window) are all non-zero
samples      channel c of a candidate whose nine bytes all lie in 1 .. 254: a clipped byte carries no noise, and a saturated flat area would
             otherwise pull the estimate to 0.  r = sum K I_c, |r| <= 8 * 253 = 2024
histogram    hist[min(|r|, 1023)] += 1: 1024 uint32 bins, all channels pooled; at most 3 * 16384^2 < 2^32 samples
record       four uint64 [n, m, sigma_q8, 0]: n = sum hist; k = max(1, (n q + 255) >> 8) with q = quantile_q8 in 1 .. 256 (0: 128, the median);
             m = the smallest bin whose cumulative count is >= k, 0 when n == 0; sigma_q8 = (256000 m + 2023) // 4047 -- sigma in 1 / 256 grey
             levels, rounded: the median of |N(0, 1)| is 0.6745, so the median of |r| is 6 * 0.6745 sigma = 4.047 sigma.
strength     noise_strength(n, m, scale, fallback, min_samples): fallback where n < min_samples, else clamp((scale m + 8) >> 4, 1, 255).
             scale in 1 .. 255 (0: 12), min_samples >= 0 (0: 1024, the blend's min_overlap).  scale = 12 gives h = 12 at m = 16, which is what the
             project's quality scene measures at its noise of +-6: h = 3.04 sigma_hat.  At m >= 340 h is 255: the clamp of the bins at 1023
             loses nothing.

The quantile's default (the median) is a choice, not a measurement.

Not here: signal-dependent (Poisson) noise, a sigma per channel or per region, a temporal estimator from registered differences.
"""
import numpy as np

BINS = 1024
QUANTILE_DEFAULT, QUANTILE_MAX = 128, 256  # a choice, not a measurement
SCALE_DEFAULT, SCALE_MAX = 12, 255
MIN_SAMPLES_DEFAULT = 1024
STRENGTH_MAX = 255
K = np.array([[1, -2, 1], [-2, 4, -2], [1, -2, 1]], dtype=np.int64)


def _planes(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a[..., None] if a.ndim == 2 else a


def _all9(ok):
    """(rows - 2, cols - 2): every one of the nine entries of the 3 x 3 window about the interior pixel holds"""
    rows, cols = ok.shape[:2]
    out = np.ones((rows - 2, cols - 2) + ok.shape[2:], dtype=bool)
    for dy in range(3):
        for dx in range(3):
            out &= ok[dy:dy + rows - 2, dx:dx + cols - 2]
    return out


def responses(image, mask):
    """-> (r (rows - 2, cols - 2, CH) int64: the mask's answer about every interior pixel, sample (same shape) bool)"""
    I = _planes(image).astype(np.int64)
    rows, cols, ch = I.shape
    assert np.asarray(mask).shape == (rows, cols) and rows >= 2 and cols >= 2 and ch in (1, 3)
    r = np.zeros((rows - 2, cols - 2, ch), dtype=np.int64)
    for dy in range(3):
        for dx in range(3):
            r += K[dy, dx] * I[dy:dy + rows - 2, dx:dx + cols - 2]
    candidate = _all9(np.asarray(mask) != 0)
    unclipped = _all9((I >= 1) & (I <= 254))
    return r, candidate[..., None] & unclipped


def histogram(image, mask):
    """-> hist (1024,) uint32"""
    r, sample = responses(image, mask)
    bins = np.minimum(np.abs(r[sample]), BINS - 1)
    return np.bincount(bins, minlength=BINS).astype(np.uint32)


def resolve(hist, quantile_q8=0):
    """-> record (4,) uint64 [n, m, sigma_q8, 0]"""
    q = int(quantile_q8) or QUANTILE_DEFAULT
    assert 1 <= q <= QUANTILE_MAX and len(hist) == BINS
    h = [int(x) for x in hist]
    n = sum(h)
    m = 0
    if n:
        k = max(1, (n * q + 255) >> 8)
        cum = 0
        for m, x in enumerate(h):
            cum += x
            if cum >= k:
                break
    return np.array([n, m, (256000 * m + 2023) // 4047, 0], dtype=np.uint64)


def noise_level(image, mask, quantile_q8=0):
    """-> dict(hist (1024,) uint32, record (4,) uint64)"""
    hist = histogram(image, mask)
    return dict(hist=hist, record=resolve(hist, quantile_q8))


def noise_strength(n, m, scale=0, fallback=12, min_samples=0):
    scale, min_samples = int(scale) or SCALE_DEFAULT, int(min_samples) or MIN_SAMPLES_DEFAULT
    assert 1 <= scale <= SCALE_MAX and min_samples >= 0 and 1 <= fallback <= STRENGTH_MAX and n >= 0 and m >= 0
    if n < min_samples:
        return int(fallback)
    return int(min(max((scale * int(m) + 8) >> 4, 1), STRENGTH_MAX))


def sigma(record):
    """the record's sigma in grey levels"""
    return int(record[2]) / 256.0
