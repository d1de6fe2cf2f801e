"""Executable definition of the temporal denoise (include/rsdsfm_denoise.h): the own frame of a solved clip averaged with its neighbours, each
rendered ALONE into the own frame's (virtual) camera, with a weight per pixel and neighbour from the mean absolute difference over a 3 x 3
patch.  The reference has no counterpart (main.cc:380-523 solves pairs one by one and never relates them); this file is the definition and the
kernel (csrc/denoise_kernels.hip) and host functions (csrc/denoise_host.hip) reproduce it bit for bit.  Every render is
tests/retime_spec_numpy.py's and tests/stabilize_crop_spec_numpy.py's, the record and the gains tests/stabilize_blend_spec_numpy.py's, imported
and unchanged.

Integers only.  W = 16; strength h 1 .. 255 (default 12, a choice); radius K 1 .. 7 (default 2): at most 14 layers.

gains        per channel G_c = blend.gains(record): clamp((sum image_c 65536 + (sum layer_c >> 1)) // sum layer_c, 16384, 262144); 65536 when
             gain_mode == 1, count < min_overlap, sum layer_c == 0, or without a record.  k_c = min(255, (G_c L_c + 32768) >> 16).
valid        v(p) = mR(p) != 0 and mL(p) != 0
error        e(p) = sum_c |R_c(p) - k_c(p)| where v(p)
patch        D(p) = sum of e(p') and N(p) = CH #{p'} over the p' of the 3 x 3 window about p that lie inside the frame and have v(p')
weight       w(p) = 16 - min(16, (16 D) // (h N)) where v(p), else 0
cell         per pixel CH + 1 uint16 [s_c, n] (the shutter's layout)
             first      cell = [16 R_c, 16] where mR != 0, else 0 (what the cells held never shows); then the layer is added
             every step s_c += w k_c, n += w                                       (n <= 16 + 14 * 16 = 240, s_c <= 61 200)
             last       the cells are not written; where n > 0 out_c = (2 s_c + n) // (2 n) (round half up), mask 1, else image 0, mask 0;
                        weight plane = n; counts = [unset: n == 0, own only: n == 16, averaged: n > 16]
no layer     first and last: the reference where mR != 0, 0 / 0 elsewhere, weight 16 or 0
frame        source 0 (the own frame) through the window with id 1 and its source plane; every other source rendered alone (id 2; through the
             occlusion test or the search when asked), blend.overlap_sums(reference, its source plane, layer) -> the record -> a step.

The sums are integers: the order of the layers does not matter.  A layer with w = 0 everywhere leaves the own frame's bytes exactly.

Not here: spatial (single-frame) denoising, patches other than 3 x 3, a noise-level estimate, moving objects (they fall back to the own pixel).
"""
import numpy as np

import retime_spec_numpy as retime
import stabilize_blend_spec_numpy as blend
import stabilize_crop_spec_numpy as crop

W = 16
STRENGTH_DEFAULT, STRENGTH_MAX = 12, 255  # a choice, not a measurement
RADIUS_DEFAULT, RADIUS_MAX = 2, 7
LAYERS_MAX = 2 * RADIUS_MAX
MIN_OVERLAP_DEFAULT = blend.MIN_OVERLAP_DEFAULT


def _planes(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a[..., None] if a.ndim == 2 else a


def gains(record, ch, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0):
    """-> list of ch integers; record None: no gain"""
    return [blend.GAIN_ONE] * ch if record is None else blend.gains(record, ch, min_overlap, gain_mode)


def gained(layer, G):
    """k (rows, cols, CH) int64"""
    lay = _planes(layer).astype(np.int64)
    return np.stack([np.minimum(255, (int(G[c]) * lay[..., c] + 32768) >> 16) for c in range(lay.shape[2])], axis=-1)


def box3(a):
    """the 3 x 3 sum about every pixel, outside the frame 0"""
    p = np.pad(a, 1)
    rows, cols = a.shape
    return sum(p[dy:dy + rows, dx:dx + cols] for dy in range(3) for dx in range(3))


def weights(ref, ref_mask, layer, layer_mask, G, strength=STRENGTH_DEFAULT):
    """-> (w (rows, cols) int64, k (rows, cols, CH) int64)"""
    assert 1 <= strength <= STRENGTH_MAX
    R = _planes(ref).astype(np.int64)
    k = gained(layer, G)
    v = (np.asarray(ref_mask) != 0) & (np.asarray(layer_mask) != 0)
    e = np.where(v, np.abs(R - k).sum(axis=-1), 0)
    D, N = box3(e), R.shape[2] * box3(v.astype(np.int64))
    w = np.where(v, W - np.minimum(W, (W * D) // np.maximum(strength * N, 1)), 0)
    return w, k


def step(cells, ref, ref_mask, layer, layer_mask, first, record=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, strength=STRENGTH_DEFAULT):
    """one layer (None, None: no layer) onto the cells ((rows, cols, CH + 1) uint16, or None with first) -> the new cells (a new array)"""
    R = _planes(ref).astype(np.int64)
    mR = np.asarray(ref_mask) != 0
    assert mR.shape == R.shape[:2] and (layer is None) == (layer_mask is None)
    if first:
        total = np.concatenate([W * R, np.full(mR.shape + (1,), W, dtype=np.int64)], axis=-1) * mR[..., None]
    else:
        assert cells.shape == R.shape[:2] + (R.shape[2] + 1,) and cells.dtype == np.uint16
        total = cells.astype(np.int64)
    if layer is not None:
        w, k = weights(ref, ref_mask, layer, layer_mask, gains(record, R.shape[2], min_overlap, gain_mode), strength)
        total = total + np.concatenate([w[..., None] * k, w[..., None]], axis=-1)
    assert total[..., -1].max() <= W * (1 + LAYERS_MAX) and total.max() <= 255 * W * (1 + LAYERS_MAX)
    return total.astype(np.uint16)


def resolve(cells, gray):
    """-> dict(image, mask, weight, counts [unset, own only, averaged])"""
    c = cells.astype(np.int64)
    s, n = c[..., :-1], c[..., -1]
    ok = n > 0
    den = np.where(ok, 2 * n, 1)
    out = np.where(ok[..., None], (2 * s + n[..., None]) // den[..., None], 0).astype(np.uint8)
    counts = [int((n == 0).sum()), int((n == W).sum()), int((n > W).sum())]
    return dict(image=out[..., 0] if gray else out, mask=ok.astype(np.uint8), weight=n.astype(np.uint8), counts=counts)


def denoise(ref, ref_mask, layers, records=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, strength=STRENGTH_DEFAULT):
    """layers: a list of 0 .. 14 (image, mask); records: None or one record (or None) per layer -> resolve's dict plus cells (after every step)"""
    assert len(layers) <= LAYERS_MAX
    steps = list(layers) if layers else [(None, None)]
    cells, trail = None, []
    for j, (image, mask) in enumerate(steps):
        cells = step(cells, ref, ref_mask, image, mask, j == 0, records[j] if records is not None and layers else None, min_overlap, gain_mode, strength)
        trail.append(cells)
    return dict(resolve(cells, np.asarray(ref).ndim == 2), cells=trail)


def denoise_frame(images, depths, Rs, ts, K, M, m, window=None, strength=STRENGTH_DEFAULT, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, occlusion=0, search_on=0,
                  tol_q16=0, mode=0, q5_mode=0, iterations=0):
    """images, depths, Rs, ts: 1 .. 15 sources, source 0 the own frame; M (nsrc, 3, 3), m (nsrc, 3): every source's pose in the target camera.
    -> denoise's dict plus ref (image, mask, source), layers [(image, mask), ...] and records (nsrc - 1, 8) uint64"""
    nsrc = len(images)
    assert 1 <= nsrc <= 1 + LAYERS_MAX
    rows, cols = np.asarray(depths[0]).shape
    window = (0, 0, rows, cols) if window is None else tuple(window)
    M, m = np.asarray(M, dtype=np.float64).reshape(-1, 3, 3), np.asarray(m, dtype=np.float64).reshape(-1, 3)
    own = np.ascontiguousarray(images[0], dtype=np.uint8)
    ref, rmask, rsource = np.zeros_like(own), np.zeros((rows, cols), dtype=np.uint8), np.zeros((rows, cols), dtype=np.uint8)
    crop.fill_from_window(ref, rmask, rsource, own, depths[0], Rs[0], ts[0], K, M[0], m[0], 1, window, mode, q5_mode, iterations)
    layers = [retime.render_layer(images[k], depths[k], Rs[k], ts[k], K, M[k], m[k], window, 2, occlusion, search_on, tol_q16, mode, q5_mode, iterations)
              for k in range(1, nsrc)]
    records = np.array([blend.overlap_sums(ref, rsource, li, lm) for li, lm in layers], dtype=np.uint64).reshape(-1, 8)
    out = denoise(ref, rmask, layers, list(records), min_overlap, gain_mode, strength)
    return dict(out, ref=(ref, rmask, rsource), layers=layers, records=records)


def neighbour_order(q, nsources, radius=RADIUS_DEFAULT):
    """the sources of frame q's denoise call: q itself, then the fill's neighbour order (nearer first, previous before next)"""
    assert 0 <= q <= nsources - 1 and 1 <= radius <= RADIUS_MAX
    out = [q]
    for d in range(1, radius + 1):
        out += [n for n in (q - d, q + d) if 0 <= n <= nsources - 1]
    return out
