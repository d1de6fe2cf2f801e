"""Executable definition of the multi-frame super-resolution (include/rsdsfm_superres.h): a frame of a solved clip on a grid S times finer than
its source, merged from the own frame and its neighbours, each rendered ALONE into the own frame's (virtual) camera on the fine grid.  A render
reports, beside the bilinear sample, the NEAREST source sample of every fine pixel and how near it fell (the proximity, 1 .. 16); the merge
weights a neighbour's nearest sample by that and by the denoise's 3 x 3 patch weight, taken on the bilinear samples.  The reference has no
counterpart (main.cc:380-523 solves pairs one by one and never relates them); this file is the definition and the kernels
(csrc/superres_kernels.hip, compiled with -ffp-contract=off) and host functions (csrc/superres_host.hip) reproduce it bit for bit.
tests/rectify_dense_spec_numpy.py, tests/stabilize_spec_numpy.py, tests/stabilize_crop_spec_numpy.py, tests/stabilize_blend_spec_numpy.py,
tests/stabilize_fill_spec_numpy.py, tests/retime_spec_numpy.py and tests/denoise_spec_numpy.py are imported and unchanged.

Positions are float64 with one rounding per operation, in the order written; everything after the render is integers.

render       one source onto orows x ocols = S rows x S cols, S 1 .. 4, both at most 16384; window (r0, c0, h, w) as in the crop stage.
             target   tx = (c0 + (X + 0.5) (w / ocols)) - 0.5, ty = (r0 + (Y + 0.5) (h / orows)) - 0.5: crop.window_targets with the OUTPUT size
             stage C  p = t, p <- t - bilinear(D, p), D on the source grid; valid iff -0.5 <= p < size - 0.5 on both axes
             taps     (i0, i1, a) per axis as the dense spec's bilinear takes them
             bil      saturate_u8 of the two lerps (the existing sample)
             near     the source byte at (a_y < 0.5 ? i0 : i1, a_x < 0.5 ? i0 : i1): the a = 0.5 tie goes to i1
             prox     d = min(a, 1 - a) per axis; 1 + (int) floor(15 ((1 - 2 d_x) (1 - 2 d_y))), 1 .. 16
             bil, near and prox are 0 where not valid, and all-zero for a source without a valid depth; a plane's mask is prox != 0.
             At S = 1 bil and prox != 0 are crop.backward_warp_window's image and mask.
accumulate   reference = the own frame's planes (R = bil, RN = near, qR = prox), layer = a neighbour's (B, Nn, qL); gains G_c and
             k(x) = min(255, (G_c x + 32768) >> 16) as in the denoise.
             v = qR != 0 and qL != 0; e = sum_c |R_c - k(B_c)| where v; D, N the 3 x 3 sums of e and of CH v inside the frame;
             w = 16 - min(16, (16 D) // (h N)) where v, else 0; u = (w qL + 8) >> 4, 0 .. 16.
             cell     CH + 1 uint16 [s_c, n] (the shutter's)
             first    cell = [qR RN_c, qR] (0 where qR = 0, whatever it held); then the layer is added
             every    s_c += u k(Nn_c), n += u                                   (n <= 16 + 14 * 16 = 240, s_c <= 61 200)
             last     cells not written; n > qR: out_c = (2 s_c + n) // (2 n); n == qR > 0: out_c = R_c (a pixel no neighbour contributed to is
                      the bilinear upscale, not a blocky nearest one); else 0.  mask = n > 0, weight plane = n,
                      counts = [unset, own only: n == qR > 0, merged: n > qR]
no layer     first and last: image R, mask qR != 0, weight qR.
frame        source 0 and every neighbour rendered alone; per neighbour blend.overlap_sums(R, (qR != 0) as the source plane, B, qL) -> the
             record -> one step.

The sums are integers: the order of the layers does not matter.  A layer with w = 0 everywhere leaves R's bytes exactly.

The proximity weight, the nearest-sample values, the 3 x 3 patch on the fine grid and the defaults (scale 2, radius 2, strength 12) are
choices, not measurements.

Not here: neighbours through the occlusion test or the search, deconvolution or sharpening of the sensor blur, non-integer scales, a fused
render-and-accumulate, fill, blend or inpaint of the result.
"""
import numpy as np

import denoise_spec_numpy as denoise
import rectify_dense_spec_numpy as dense
import retime_spec_numpy as retime  # noqa: F401
import stabilize_blend_spec_numpy as blend
import stabilize_crop_spec_numpy as crop  # noqa: F401
import stabilize_spec_numpy as stab

W = denoise.W
PROX_MAX = 16
SCALE_DEFAULT, SCALE_MAX = 2, 4  # a choice, not a measurement
STRENGTH_DEFAULT, STRENGTH_MAX = denoise.STRENGTH_DEFAULT, denoise.STRENGTH_MAX
RADIUS_DEFAULT, RADIUS_MAX = denoise.RADIUS_DEFAULT, denoise.RADIUS_MAX
LAYERS_MAX = denoise.LAYERS_MAX
MIN_OVERLAP_DEFAULT = denoise.MIN_OVERLAP_DEFAULT
SIZE_MAX = 16384

_planes = denoise._planes
gains = denoise.gains
gained = denoise.gained
box3 = denoise.box3
neighbour_order = denoise.neighbour_order


# ---------------------------------------------------------------------------------------------------
# the render
# ---------------------------------------------------------------------------------------------------
def fine_targets(window, rows, cols, scale):
    """-> tx, ty (scale rows, scale cols) float64: crop.window_targets with the output size in place of the frame's"""
    r0, c0, h, w = (int(v) for v in window)
    orows, ocols = scale * rows, scale * cols
    assert 1 <= scale <= SCALE_MAX and orows <= SIZE_MAX and ocols <= SIZE_MAX
    assert h >= 1 and w >= 1 and r0 >= 0 and c0 >= 0 and r0 + h <= rows and c0 + w <= cols
    iy, ix = np.mgrid[0:orows, 0:ocols].astype(np.float64)
    sx, sy = np.float64(w) / np.float64(ocols), np.float64(h) / np.float64(orows)
    return (np.float64(c0) + (ix + 0.5) * sx) - 0.5, (np.float64(r0) + (iy + 0.5) * sy) - 0.5


def tap(p, n):
    """the dense spec's taps of position p on an axis of n samples -> (i0, i1, a)"""
    c = dense._clamp(p, n)
    i0 = np.floor(c).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), c - i0


def proximity(ax, ay):
    """-> int64, 1 .. 16: 16 on a source sample, 1 half way between two on either axis"""
    dx, dy = np.minimum(ax, 1.0 - ax), np.minimum(ay, 1.0 - ay)
    return 1 + np.floor(15.0 * ((1.0 - 2.0 * dx) * (1.0 - 2.0 * dy))).astype(np.int64)


def sample_planes(image, px, py, valid):
    """the three planes at positions (px, py) of the source grid -> (bil, near, prox) uint8"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    rows, cols = image.shape[:2]
    with np.errstate(all="ignore"):
        x0, x1, ax = tap(px, cols)
        y0, y1, ay = tap(py, rows)
        bil = dense.saturate_u8(dense.bilinear(image, px, py))
        near = image[np.where(ay < 0.5, y0, y1), np.where(ax < 0.5, x0, x1)]
        prox = proximity(ax, ay)
    keep = valid[..., None] if image.ndim == 3 else valid
    return np.where(keep, bil, 0).astype(np.uint8), np.where(keep, near, 0).astype(np.uint8), np.where(valid, prox, 0).astype(np.uint8)


def fine_positions(D, iterations, window, scale):
    rows, cols = D.shape[:2]
    tx, ty = fine_targets(window, rows, cols, scale)
    px, py = tx, ty
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            d = dense.bilinear(D, px, py)
            px, py = tx - d[..., 0], ty - d[..., 1]
        valid = (px >= -0.5) & (px < cols - 0.5) & (py >= -0.5) & (py < rows - 0.5)
    return px, py, valid


def render(image, depth, R, t, K, M, m, scale=SCALE_DEFAULT, window=None, mode=0, q5_mode=0, iterations=0):
    """one source alone onto the fine grid -> dict(bil, near, prox)"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    it = iterations if iterations else dense.DEFAULT_ITERATIONS
    assert 1 <= it <= 16
    z = np.asarray(depth, dtype=np.float64)
    rows, cols = z.shape
    window = (0, 0, rows, cols) if window is None else tuple(window)
    fine = (scale * rows, scale * cols)
    if not dense.inverse_depth(z).any():  # no valid pixel: all-zero outputs
        zero = np.zeros(fine + image.shape[2:], dtype=np.uint8)
        return dict(bil=zero, near=zero.copy(), prox=np.zeros(fine, dtype=np.uint8))
    _, _, D = stab.forward_map(dense.fill_depth(z), R, t, K[0], K[1], K[2], K[3], M, m, mode, q5_mode)
    px, py, valid = fine_positions(D, it, window, scale)
    bil, near, prox = sample_planes(image, px, py, valid)
    return dict(bil=bil, near=near, prox=prox)


# ---------------------------------------------------------------------------------------------------
# the accumulate
# ---------------------------------------------------------------------------------------------------
def weights(ref, ref_prox, layer, layer_prox, G, strength=STRENGTH_DEFAULT):
    """-> (u (rows, cols) int64: the patch weight times the layer's proximity, w (rows, cols) int64: the patch weight alone)"""
    w, _ = denoise.weights(ref, ref_prox, layer, layer_prox, G, strength)
    return (w * np.asarray(layer_prox).astype(np.int64) + 8) >> 4, w


def step(cells, ref, ref_near, ref_prox, layer, layer_near, layer_prox, first, record=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, strength=STRENGTH_DEFAULT):
    """one layer (None, None, None: no layer) onto the cells ((rows, cols, CH + 1) uint16, or None with first) -> the new cells (a new array)"""
    RN = _planes(ref_near).astype(np.int64)
    qR = np.asarray(ref_prox).astype(np.int64)
    assert qR.shape == RN.shape[:2] and qR.max(initial=0) <= PROX_MAX
    if first:
        total = np.concatenate([qR[..., None] * RN, qR[..., None]], axis=-1)
    else:
        assert cells.shape == RN.shape[:2] + (RN.shape[2] + 1,) and cells.dtype == np.uint16
        total = cells.astype(np.int64)
    if layer is not None:
        assert np.asarray(layer_prox).max(initial=0) <= PROX_MAX
        G = gains(record, RN.shape[2], min_overlap, gain_mode)
        u, _ = weights(ref, ref_prox, layer, layer_prox, G, strength)
        total = total + np.concatenate([u[..., None] * gained(layer_near, G), u[..., None]], axis=-1)
    assert total[..., -1].max() <= W * (1 + LAYERS_MAX) and total.max() <= 255 * W * (1 + LAYERS_MAX)
    return total.astype(np.uint16)


def resolve(cells, ref, ref_prox):
    """-> dict(image, mask, weight, counts [unset, own only, merged])"""
    R = _planes(ref).astype(np.int64)
    qR = np.asarray(ref_prox).astype(np.int64)
    c = cells.astype(np.int64)
    s, n = c[..., :-1], c[..., -1]
    merged, own = n > qR, (n == qR) & (qR > 0)
    den = np.where(merged, 2 * n, 1)
    out = np.where(merged[..., None], (2 * s + n[..., None]) // den[..., None], np.where(own[..., None], R, 0)).astype(np.uint8)
    counts = [int((~merged & ~own).sum()), int(own.sum()), int(merged.sum())]
    return dict(image=out[..., 0] if np.asarray(ref).ndim == 2 else out, mask=(n > 0).astype(np.uint8), weight=n.astype(np.uint8), counts=counts)


def accumulate(ref, ref_near, ref_prox, layers, records=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, strength=STRENGTH_DEFAULT):
    """layers: a list of 0 .. 14 (bil, near, prox); records: None or one record (or None) per layer -> resolve's dict plus cells (after every step)"""
    assert len(layers) <= LAYERS_MAX
    steps = list(layers) if layers else [(None, None, None)]
    cells, trail = None, []
    for j, (b, nn, q) in enumerate(steps):
        cells = step(cells, ref, ref_near, ref_prox, b, nn, q, j == 0, records[j] if records is not None and layers else None, min_overlap, gain_mode, strength)
        trail.append(cells)
    return dict(resolve(cells, ref, ref_prox), cells=trail)


# ---------------------------------------------------------------------------------------------------
# the frame
# ---------------------------------------------------------------------------------------------------
def superres_frame(images, depths, Rs, ts, K, M, m, scale=SCALE_DEFAULT, window=None, strength=STRENGTH_DEFAULT, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, mode=0,
                   q5_mode=0, iterations=0):
    """images, depths, Rs, ts: 1 .. 15 sources, source 0 the own frame; M (nsrc, 3, 3), m (nsrc, 3): every source's pose in the target camera.
    -> accumulate's dict plus planes [dict(bil, near, prox), ...] and records (nsrc - 1, 8) uint64"""
    nsrc = len(images)
    assert 1 <= nsrc <= 1 + LAYERS_MAX
    M, m = np.asarray(M, dtype=np.float64).reshape(-1, 3, 3), np.asarray(m, dtype=np.float64).reshape(-1, 3)
    planes = [render(images[k], depths[k], Rs[k], ts[k], K, M[k], m[k], scale, window, mode, q5_mode, iterations) for k in range(nsrc)]
    own = planes[0]
    source = (own["prox"] != 0).astype(np.uint8)
    records = np.array([blend.overlap_sums(own["bil"], source, p["bil"], p["prox"]) for p in planes[1:]], dtype=np.uint64).reshape(-1, 8)
    out = accumulate(own["bil"], own["near"], own["prox"], [(p["bil"], p["near"], p["prox"]) for p in planes[1:]], list(records), min_overlap, gain_mode, strength)
    return dict(out, planes=planes, records=records)
