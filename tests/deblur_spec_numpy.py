"""Executable definition of the sharpness transfer (include/rsdsfm_deblur.h): a frame of a solved clip that the camera's shake blurred takes
pixels from its registered neighbours where a neighbour is sharper (Matsushita, Ofek, Ge, Tang, Shum, "Full-frame video stabilization with
motion inpainting", 2006, section 5).  The reference has no counterpart (main.cc:380-523 solves pairs one by one and never relates them); this
file is the definition and the kernels (csrc/deblur_kernels.hip) and host functions (csrc/deblur_host.hip) reproduce it bit for bit.  The gains,
the gained bytes, the cells and their resolve are tests/denoise_spec_numpy.py's, the record tests/stabilize_blend_spec_numpy.py's, the renders
tests/retime_spec_numpy.py's and tests/stabilize_crop_spec_numpy.py's, imported and unchanged.

Integers only.  W = 16; strength h 1 .. 255 (default 24); margin 0 .. 64 sixteenths (default 4); tau <= 32; radius K 1 .. 3 (default 2); at
most 7 layers.  All four defaults are choices, not measurements.

gains        G_c and k_c = min(255, (G_c L_c + 32768) >> 16) as the denoise defines them (same gain_mode, min_overlap)
valid        v(p) = mR(p) != 0 and mL(p) != 0
luma         Y_R(p) = sum_c R_c(p), Y_L(p) = sum_c k_c(p)                                              (<= 765)
sharpness    T = [pairs, A_R, A_L, 0] (uint64): over every p with v(p) and each forward neighbour q in {p + (0, 1), p + (1, 0)} inside the frame
             with v(q): pairs += 1, A_R += (Y_R(p) - Y_R(q))^2, A_L += (Y_L(p) - Y_L(q))^2 -- the same support for both images
tau          0 when pairs < min_pairs or 16 A_L <= (16 + margin) A_R, else min(32, (16 (A_L - A_R)) // max(A_R, 1))
gate         D(p) = |sum (Y_R - Y_L)(p')| and N(p) = CH #{p'} over the p' of the 3 x 3 window about p inside the frame with v(p');
             w(p) = 16 - min(16, (16 D) // (h N)) where v(p), else 0; gate_mode 1: w = 16 wherever v
cell         the denoise's: first [16 R_c, 16] where mR != 0; every step u = (w tau + 8) >> 4, s_c += u k_c, n += u (n <= 16 + 7 * 32 = 240);
             last out_c = (2 s_c + n) // (2 n), mask 1 where n > 0; weight plane n; counts [unset: n == 0, own only: n == 16, transferred: n > 16]
frame        the denoise's frame with a sharpness record per neighbour between the overlap record and the step

Consequences: every tau = 0 -> the own frame's bytes and mask exactly; the order of the layers changes no byte; tau = 16 -> u = w.

Not here: deconvolution or any single-frame sharpening, sharpness per scanline band, gates wider than 3 x 3, the mover flag in the gate.
"""
import numpy as np

import denoise_spec_numpy as dn
import retime_spec_numpy as retime
import stabilize_blend_spec_numpy as blend
import stabilize_crop_spec_numpy as crop

W = dn.W
STRENGTH_DEFAULT, STRENGTH_MAX = 24, 255  # a choice, not a measurement
MARGIN_DEFAULT, MARGIN_MAX = 4, 64        # sixteenths; a choice
TAU_MAX = 32                              # a choice
RADIUS_DEFAULT, RADIUS_MAX = 2, 3         # a choice
LAYERS_MAX = 7
MIN_OVERLAP_DEFAULT = dn.MIN_OVERLAP_DEFAULT
MIN_PAIRS_DEFAULT = 1024
BIAS = 765


def margin_value(abi_margin):
    """the C ABI's margin word: -1 'none' (0), 0 the default, 1 .. 64 itself"""
    return 0 if abi_margin < 0 else MARGIN_DEFAULT if abi_margin == 0 else int(abi_margin)


def lumas(ref, ref_mask, layer, layer_mask, G):
    """-> (v bool, Y_R, Y_L int64 (rows, cols), k (rows, cols, CH) int64)"""
    R = dn._planes(ref).astype(np.int64)
    k = dn.gained(layer, G)
    v = (np.asarray(ref_mask) != 0) & (np.asarray(layer_mask) != 0)
    return v, R.sum(axis=-1), k.sum(axis=-1), k


def sharpness(ref, ref_mask, layer, layer_mask, record=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0):
    """-> T (4,) uint64 [pairs, A_R, A_L, 0]"""
    ch = dn._planes(ref).shape[2]
    v, YR, YL, _ = lumas(ref, ref_mask, layer, layer_mask, dn.gains(record, ch, min_overlap, gain_mode))
    pairs = a_r = a_l = 0
    for sl_p, sl_q in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))), ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
        both = v[sl_p] & v[sl_q]
        pairs += int(both.sum())
        a_r += int((((YR[sl_p] - YR[sl_q]) ** 2) * both).sum())
        a_l += int((((YL[sl_p] - YL[sl_q]) ** 2) * both).sum())
    return np.array([pairs, a_r, a_l, 0], dtype=np.uint64)


def tau(T, margin=MARGIN_DEFAULT, min_pairs=MIN_PAIRS_DEFAULT):
    """the layer factor from a sharpness record; margin 0 .. 64 (the value, not the ABI's word), min_pairs >= 1"""
    assert 0 <= margin <= MARGIN_MAX and min_pairs >= 0
    pairs, a_r, a_l = int(T[0]), int(T[1]), int(T[2])
    if pairs < min_pairs or 16 * a_l <= (16 + margin) * a_r:
        return 0
    return min(TAU_MAX, (16 * (a_l - a_r)) // max(a_r, 1))


def gate(v, YR, YL, ch, strength=STRENGTH_DEFAULT, gate_mode=0):
    """-> w (rows, cols) int64"""
    assert 1 <= strength <= STRENGTH_MAX and gate_mode in (0, 1)
    if gate_mode == 1:
        return np.where(v, W, 0).astype(np.int64)
    D = np.abs(dn.box3(np.where(v, YR - YL, 0)))
    N = ch * dn.box3(v.astype(np.int64))
    return np.where(v, W - np.minimum(W, (W * D) // np.maximum(strength * N, 1)), 0)


def step(cells, ref, ref_mask, layer, layer_mask, first, t=0, record=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, strength=STRENGTH_DEFAULT, gate_mode=0):
    """one layer (None, None: no layer) with the factor t onto the cells -> the new cells (a new array)"""
    R = dn._planes(ref).astype(np.int64)
    mR = np.asarray(ref_mask) != 0
    assert mR.shape == R.shape[:2] and (layer is None) == (layer_mask is None) and 0 <= t <= TAU_MAX
    if first:
        total = np.concatenate([W * R, np.full(mR.shape + (1,), W, dtype=np.int64)], axis=-1) * mR[..., None]
    else:
        assert cells.shape == R.shape[:2] + (R.shape[2] + 1,) and cells.dtype == np.uint16
        total = cells.astype(np.int64)
    if layer is not None:
        v, YR, YL, k = lumas(ref, ref_mask, layer, layer_mask, dn.gains(record, R.shape[2], min_overlap, gain_mode))
        u = (gate(v, YR, YL, R.shape[2], strength, gate_mode) * t + 8) >> 4
        total = total + np.concatenate([u[..., None] * k, u[..., None]], axis=-1)
    assert total[..., -1].max() <= W + LAYERS_MAX * TAU_MAX and total.max() <= 255 * (W + LAYERS_MAX * TAU_MAX)
    return total.astype(np.uint16)


def deblur(ref, ref_mask, layers, records=None, sharps=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, strength=STRENGTH_DEFAULT, margin=MARGIN_DEFAULT,
           min_pairs=MIN_PAIRS_DEFAULT, gate_mode=0):
    """layers: a list of 0 .. 7 (image, mask); records: None or one 8-word record (or None) per layer; sharps: None (every layer's sharpness
    record is computed) or one 4-word record per layer -> denoise's resolve dict plus cells (after every step), sharps (n, 4) uint64, taus"""
    assert len(layers) <= LAYERS_MAX
    rec = lambda j: records[j] if records is not None else None
    if sharps is None:
        sharps = [sharpness(ref, ref_mask, li, lm, rec(j), min_overlap, gain_mode) for j, (li, lm) in enumerate(layers)]
    taus = [tau(T, margin, min_pairs) for T in sharps]
    cells, trail = None, []
    for j, (image, mask) in enumerate(list(layers) if layers else [(None, None)]):
        cells = step(cells, ref, ref_mask, image, mask, j == 0, taus[j] if layers else 0, rec(j) if layers else None, min_overlap, gain_mode, strength, gate_mode)
        trail.append(cells)
    return dict(dn.resolve(cells, np.asarray(ref).ndim == 2), cells=trail, sharps=np.array(sharps, dtype=np.uint64).reshape(-1, 4), taus=taus)


def deblur_frame(images, depths, Rs, ts, K, M, m, window=None, strength=STRENGTH_DEFAULT, margin=MARGIN_DEFAULT, min_pairs=MIN_PAIRS_DEFAULT, gate_mode=0,
                 min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, occlusion=0, search_on=0, tol_q16=0, mode=0, q5_mode=0, iterations=0):
    """images, depths, Rs, ts: 1 .. 8 sources, source 0 the own frame; M (nsrc, 3, 3), m (nsrc, 3): every source's pose in the target camera.
    -> deblur's dict plus ref (image, mask, source), layers [(image, mask), ...] and records (nsrc - 1, 8) uint64"""
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
    out = deblur(ref, rmask, layers, list(records), None, min_overlap, gain_mode, strength, margin, min_pairs, gate_mode)
    return dict(out, ref=(ref, rmask, rsource), layers=layers, records=records)


def neighbour_order(q, nsources, radius=RADIUS_DEFAULT):
    """the sources of frame q's call: q itself, then the fill's neighbour order (nearer first, previous before next)"""
    assert 1 <= radius <= RADIUS_MAX
    return dn.neighbour_order(q, nsources, radius)


def box_blur(frame, width):
    """a frame's rounded horizontal box mean over `width` (odd) columns with replicated edges: synth.render_sequence's blur, for the tests' clips"""
    assert width >= 1 and width % 2 == 1
    if width == 1:
        return np.ascontiguousarray(frame, dtype=np.uint8)
    a = np.asarray(frame).astype(np.int64)
    h = width // 2
    idx = np.clip(np.arange(-h, a.shape[1] + h), 0, a.shape[1] - 1)
    p = a[:, idx]
    s = sum(p[:, d:d + a.shape[1]] for d in range(width))
    return ((2 * s + width) // (2 * width)).astype(np.uint8)
