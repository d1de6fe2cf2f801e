"""Executable definition of the synthetic shutter (include/rsdsfm_shutter.h): a frame of a solved clip EXPOSED over a window of time, the mean
of the scene rendered at S sub-instants along the camera path.  The reference has no counterpart (main.cc:380-523 solves pairs one by one and
never relates them); this file is the definition and the kernel (csrc/shutter_kernels.hip) and host functions (csrc/shutter_host.hip, compiled
with -ffp-contract=off) reproduce it bit for bit.  Every render and merge is tests/retime_spec_numpy.py's, imported and unchanged.

shutter_times  u_j = (j + 0.5) / S - 0.5, t_j = t + shutter * u_j for j = 0 .. S - 1 (float64, one rounding per operation, in this order);
               t_j is kept iff 0 <= t_j <= nsources - 1.  S = 1: t_0 == t bitwise; shutter = 0: every t_j == t.  At least one is kept.
cell           per pixel channels + 1 uint16: [s_b, s_g, s_r, n] (BGR) or [s, n] (gray).  64 * 255 = 16 320: nothing overflows.
accumulate     one sample, flags first and last.  A pixel counts iff its mask byte != 0.  first: cell = the pixel and n = 1, or 0 where the mask
               is 0 (what the cells held never shows).  Not first: s_c += v_c, n += 1 where the mask is set.  Not last: the cells are written.
               last: the cells are not written; resolve: where n >= min_samples out_c = (2 s_c + n) // (2 n) (the mean, round half up), mask 1,
               else image 0, mask 0; coverage = n; counts = [unset: n < min_samples, partial: min_samples <= n < nsamples, full: n == nsamples].
expose         a list of samples in order, first on the first and last on the last.  Integers: the order of the samples does not matter.
shutter_frame  for every kept sub-instant retime.retime_poses(t_j) and retime.retime_frame; the samples exposed with nsamples = the kept count
               and min_samples = min(min_samples, kept): a window clipped at the clip's end asks of a pixel what it can give.

Not here: weighted (non-box) shutters, rolling-shutter re-synthesis, fill or inpaint of the exposed frame.
"""
import numpy as np

import retime_spec_numpy as retime

SAMPLES_MAX = 64
SHUTTER_DEFAULT, SAMPLES_DEFAULT, MIN_SAMPLES_DEFAULT = 0.5, 8, 1  # choices, not measurements


def shutter_times(t, shutter, samples, nsources):
    """-> the kept sub-instants, a list of float64 in order"""
    t, shutter = np.float64(t), np.float64(shutter)
    assert 1 <= samples <= SAMPLES_MAX and nsources >= 1
    assert np.isfinite(shutter) and 0 <= shutter <= nsources - 1 and np.isfinite(t) and 0 <= t <= nsources - 1
    kept = []
    for j in range(samples):
        u = (np.float64(j) + np.float64(0.5)) / np.float64(samples) - np.float64(0.5)
        tj = t + shutter * u
        if 0 <= tj <= nsources - 1:
            kept.append(tj)
    assert len(kept) >= 1
    return kept


def accumulate(cells, image, mask, first):
    """cells (rows, cols, channels + 1) uint16 or None (first only); the sample's image (rows, cols[, 3]) uint8 and mask (rows, cols) uint8
    -> the new cells (a new array)"""
    img = np.ascontiguousarray(image, dtype=np.uint8)
    m = np.asarray(mask) != 0
    assert m.shape == img.shape[:2]
    v = img.reshape(m.shape + (-1,)).astype(np.int64)
    add = np.concatenate([v, np.ones(m.shape + (1,), dtype=np.int64)], axis=-1) * m[..., None]
    if first:
        return add.astype(np.uint16)
    assert cells.shape == add.shape and cells.dtype == np.uint16
    total = cells.astype(np.int64) + add
    assert total[..., -1].max() <= SAMPLES_MAX and total.max() <= SAMPLES_MAX * 255
    return total.astype(np.uint16)


def resolve(cells, nsamples, min_samples, gray):
    """-> dict(image, mask, coverage, counts [unset, partial, full])"""
    assert 1 <= min_samples <= nsamples <= SAMPLES_MAX
    c = cells.astype(np.int64)
    s, n = c[..., :-1], c[..., -1]
    ok = n >= min_samples
    den = np.where(ok, 2 * n, 1)
    out = np.where(ok[..., None], (2 * s + n[..., None]) // den[..., None], 0).astype(np.uint8)
    counts = [int((~ok).sum()), int((ok & (n < nsamples)).sum()), int((n == nsamples).sum())]
    return dict(image=out[..., 0] if gray else out, mask=ok.astype(np.uint8), coverage=n.astype(np.uint8), counts=counts)


def expose(samples, min_samples=MIN_SAMPLES_DEFAULT, nsamples=None):
    """samples: a list of (image, mask); nsamples None: len(samples) -> resolve's dict"""
    assert 1 <= len(samples) <= SAMPLES_MAX
    cells = None
    for j, (image, mask) in enumerate(samples):
        cells = accumulate(cells, image, mask, j == 0)
    return resolve(cells, len(samples) if nsamples is None else nsamples, min_samples, np.asarray(samples[0][0]).ndim == 2)


def shutter_frame(frames, depths, Rs, ts, K, A, c, A_path, c_path, scales, t, shutter=SHUTTER_DEFAULT, samples=SAMPLES_DEFAULT, min_samples=MIN_SAMPLES_DEFAULT,
                  window=None, threshold=retime.THRESHOLD_DEFAULT, occlusion=0, search_on=0, tol_q16=0, mode=0, q5_mode=0, iterations=0):
    """frames, depths, Rs, ts: the clip's sources (nsources = len(depths)); A, c, A_path, c_path, scales: retime_poses'.
    -> resolve's dict plus times (the kept sub-instants) and samples [(image, mask), ...]"""
    nsources = len(depths)
    assert 1 <= min_samples <= samples
    times = shutter_times(t, shutter, samples, nsources)
    rendered = []
    for tj in times:
        p = retime.retime_poses(A, c, A_path, c_path, scales, nsources, tj)
        src = p["sources"]
        r = retime.retime_frame([frames[n] for n in src], [depths[n] for n in src], [Rs[n] for n in src], [ts[n] for n in src], K, p["M"], p["m"], p["weight"], window,
                                threshold, occlusion, search_on, tol_q16, mode, q5_mode, iterations)
        rendered.append((r["image"], r["mask"]))
    return dict(expose(rendered, min(min_samples, len(times))), times=times, samples=rendered)
