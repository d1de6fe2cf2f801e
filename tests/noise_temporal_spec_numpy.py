"""Executable definition of the temporal noise curve (include/rsdsfm_noise_temporal.h): a frame's noise measured from the differences to its
REGISTERED NEIGHBOURS, in the noise curve's 36-word format, so that every consumer of a curve takes it unchanged.  The noise curve
(tests/noise_curve_spec_numpy.py) applies Immerkaer's 3 x 3 mask to ONE frame and so assumes that most of the frame is smooth; on a textured
frame it measures the texture.  The difference of two registered renders of a static scene holds no texture, only the noise of both and the
registration's residue: exactly what the temporal weight compares against its strength.  The kernel (csrc/noise_temporal_kernels.hip) and host
functions (csrc/noise_temporal_host.hip) reproduce this file bit for bit.  tests/denoise_spec_numpy.py, tests/noise_curve_spec_numpy.py and
tests/stabilize_blend_spec_numpy.py are imported unchanged.

Integers only.

gains        G and k = gained(L, G) exactly as in the denoise (denoise_spec_numpy.gains, gained)
valid        v(p) = mR(p) != 0 and mL(p) != 0
error        e(p) = sum_c |R_c(p) - k_c(p)| where v(p), else 0
clipped      x(p) = v(p) and any byte of R(p) or of L(p) BEFORE the gain is 0 or 255
patch        D, C, X = the 3 x 3 sums of e, v, x about p, 0 outside the frame
sample       p is a sample iff C = 9 and X = 0: a full window (so p is an interior pixel) with nothing saturated in it
bin          N = 9 CH; bin = (918 D + 128 N) // (256 N): the patch mean D / N times 918 / 256, rounded half up.  D <= 27 * 255 = 6885, so the
             product fits 32 bits, and bin <= 914 < 1024: no clamp
band         level(R(p)) >> 5 with the consumers' level: the byte (gray) or (b + g + r + 1) // 3 (BGR)
histogram    hist[band][bin] += 1, the noise curve's 8 x 1024 uint32; a frame's histogram is the SUM over its neighbours: integers, so the
             order of the neighbours and the scheduling do not matter
curve        noise_curve_spec_numpy.resolve(hist, quantile_q8), unchanged: nine rows [n, m, sigma_q8, 0]
frame        the denoise curve frame's definition with the curve taken from the summed pair histograms of all the frame's neighbours in place
             of the own render's, resolved before the first accumulate.  One source: the histogram is empty, row 8 has n = 0 and every strength
             is the fallback -- the existing rule.

918 / 256 = 3.586 is derived, not tuned.  Immerkaer's record has m = 0.6745 * 6 sigma = 4.047 sigma (the median of |N(0, 36 sigma^2)|).  For
equal, independent Gaussian noise of sigma in both frames d = R - k is N(0, 2 sigma^2) and E|d| = 2 sigma / sqrt(pi) = 1.128 sigma; the patch
mean over 9 CH differences concentrates on it, and 4.047 / 1.128 = 3.586.  So m lives on the existing scale: sigma_q8 and
h = (scale m + 8) >> 4 keep their meaning.  Measured on denoise_cases.shift_clip (uniform noise +-2 .. +-20, BGR and gray, four seeds):
sigma-hat / sigma-true in 0.991 .. 1.057 (tests/test_noise_temporal_cpu.py), where the frame's own spatial curve gives 4.8 .. 40.5.

Not here: the temporal curve fed to the sharpen stage (the noise after denoising is not the noise measured before it), a curve consumer for
the super-resolution and the sharpness transfer, histograms pooled across the frames of a clip, a fallback to the spatial curve when the
overlap is too small.
"""
import numpy as np

import denoise_spec_numpy as temporal
import noise_curve_spec_numpy as curve_spec
import stabilize_blend_spec_numpy as blend

BANDS, BINS, BAND_SHIFT = curve_spec.BANDS, curve_spec.BINS, curve_spec.BAND_SHIFT
MIN_OVERLAP_DEFAULT = blend.MIN_OVERLAP_DEFAULT
BIN_NUM, BIN_SHIFT = 918, 8  # 918 / 256 = 3.586 = 4.047 / 1.128 (above)
D_MAX = 27 * 255
assert BIN_NUM * D_MAX + 128 * 27 < 2 ** 32 and (BIN_NUM * D_MAX + 128 * 27) // (256 * 27) == 914 and (BIN_NUM * D_MAX // 3 + 128 * 9) // (256 * 9) == 914


def pair_terms(ref, ref_mask, layer, layer_mask, record=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0):
    """-> dict(sample (rows, cols) bool, bin, band (rows, cols) int64)"""
    R = temporal._planes(ref).astype(np.int64)
    L = temporal._planes(layer).astype(np.int64)
    ch = R.shape[2]
    k = temporal.gained(layer, temporal.gains(record, ch, min_overlap, gain_mode))
    v = (np.asarray(ref_mask) != 0) & (np.asarray(layer_mask) != 0)
    e = np.where(v, np.abs(R - k).sum(axis=-1), 0)
    x = v & (((R == 0) | (R == 255)).any(axis=-1) | ((L == 0) | (L == 255)).any(axis=-1))
    D, C, X = temporal.box3(e), temporal.box3(v.astype(np.int64)), temporal.box3(x.astype(np.int64))
    N = 9 * ch
    return dict(sample=(C == 9) & (X == 0), bin=(BIN_NUM * D + 128 * N) // (256 * N), band=curve_spec.pixel_levels(ref) >> BAND_SHIFT)


def pair_histogram(ref, ref_mask, layer, layer_mask, record=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0):
    """-> hist (8, 1024) uint32 of one neighbour"""
    t = pair_terms(ref, ref_mask, layer, layer_mask, record, min_overlap, gain_mode)
    s = t["sample"]
    assert not s.any() or t["bin"][s].max() < BINS
    key = (t["band"][s] << 10) | t["bin"][s]
    return np.bincount(key, minlength=BANDS * BINS).astype(np.uint32).reshape(BANDS, BINS)


def frame_histogram(ref, ref_mask, layers, records=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0):
    """the sum over the layers [(image, mask), ...]; records: None or one record (or None) per layer -> hist (8, 1024) uint32"""
    hist = np.zeros((BANDS, BINS), dtype=np.uint32)
    for j, (image, mask) in enumerate(layers):
        hist = hist + pair_histogram(ref, ref_mask, image, mask, records[j] if records is not None else None, min_overlap, gain_mode)
    return hist.astype(np.uint32)


def resolve(hist, quantile_q8=0):
    """-> curve (9, 4) uint64: noise_curve_spec_numpy.resolve"""
    return curve_spec.resolve(hist, quantile_q8)


def noise_temporal(ref, ref_mask, layers, records=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, quantile_q8=0):
    """-> dict(hist (8, 1024) uint32, curve (9, 4) uint64)"""
    hist = frame_histogram(ref, ref_mask, layers, records, min_overlap, gain_mode)
    return dict(hist=hist, curve=resolve(hist, quantile_q8))


def denoise_temporal(ref, ref_mask, layers, records=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, strength=temporal.STRENGTH_DEFAULT, quantile_q8=0, scale=0,
                     min_samples=0, band_min_samples=0, spatial=None):
    """the curve from all the layers, then noise_curve_spec_numpy.denoise on it (strength: the fallback); spatial: None or
    dict(strength, target, search) for the top-up on the same curve -> denoise's dict plus hist, curve, lut (and support, spatial_counts)"""
    n = noise_temporal(ref, ref_mask, layers, records, min_overlap, gain_mode, quantile_q8)
    lut = curve_spec.strengths(n["curve"], scale, strength, min_samples, band_min_samples)
    out = dict(curve_spec.denoise(ref, ref_mask, layers, lut, records, min_overlap, gain_mode), hist=n["hist"], curve=n["curve"], lut=lut)
    if spatial is not None:
        slut = curve_spec.strengths(n["curve"], scale, spatial["strength"], min_samples, band_min_samples)
        top = curve_spec.denoise_spatial(out["image"], out["mask"], slut, out["weight"], spatial["target"], spatial["search"])
        out.update(temporal_image=out["image"], image=top["image"], support=top["support"], spatial_counts=top["counts"])
    return out


def denoise_temporal_frame(images, depths, Rs, ts, K, M, m, window=None, strength=temporal.STRENGTH_DEFAULT, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, occlusion=0,
                           search_on=0, tol_q16=0, mode=0, q5_mode=0, iterations=0, quantile_q8=0, scale=0, min_samples=0, band_min_samples=0, spatial=None):
    """denoise_spec_numpy.denoise_frame's renders and records, then denoise_temporal -> its dict plus ref, layers and records"""
    r = temporal.denoise_frame(images, depths, Rs, ts, K, M, m, window, strength, min_overlap, gain_mode, occlusion, search_on, tol_q16, mode, q5_mode, iterations)
    ref, rmask, _ = r["ref"]
    out = denoise_temporal(ref, rmask, r["layers"], list(r["records"]), min_overlap, gain_mode, strength, quantile_q8, scale, min_samples, band_min_samples, spatial)
    return dict(out, ref=r["ref"], layers=r["layers"], records=r["records"])
