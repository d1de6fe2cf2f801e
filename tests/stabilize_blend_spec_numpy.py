"""Executable definition of the stabiliser's seam blend (include/rsdsfm_stabilize_blend.h): the photometry at the seam between the own frame
and what the border fill takes from its neighbours -- one gain per candidate and channel, matched on the overlap, and a linear feather over
the T pixels of the own frame next to its empty band.  The reference has no counterpart (main.cc:380-523 solves pairs one by one and never
relates them); this file is the definition and the kernels (csrc/stabilize_blend_kernels.hip) and host functions
(csrc/stabilize_blend_host.hip) reproduce it bit for bit.  tests/stabilize_crop_spec_numpy.py and what it imports are unchanged; the renders
are its functions.

Integers only.

seam_distance   uint8 plane: 0 where mask == 0, elsewhere min(T, the chessboard distance max(|dy|, |dx|) to the nearest empty pixel of the
                frame).  The frame's own edge is not a hole (the crop's margin has the same convention).  Written the separable way the
                kernels take: row_distance h(y, x) = the distance along the row to the nearest empty pixel, capped at T, then
                d(y, x) = min over |dy| <= T - 1, inside the frame, of max(|dy|, h(y + dy, x)).
overlap_sums    8 uint64 [count, sum image_c (c < CH), sum layer_c (c < CH), 0 ...] over the pixels with source == 1 (the own frame's, not
                yet blended) and layer_mask != 0.
gains           per channel G_c = clamp((sum image_c 65536 + (sum layer_c >> 1)) // sum layer_c, GAIN_MIN, GAIN_MAX), in 1 / 65536;
                GAIN_ONE when gain_mode == 1 (off), count < min_overlap or sum layer_c == 0.  sum image_c 65536 < 2^52 at 16384 x 16384.
blend_layer     in place, per pixel with layer_mask != 0 and k_c = min(255, (G_c layer_c + 32768) >> 16):
                  source == 0                 image = k, mask = 1, source = source_id                                       (filled)
                  source == 1 and dist < T    image_c = (dist image_c + (T - dist) k_c + (T >> 1)) // T, source = source_id  (blended)
                  otherwise                   nothing (deep inside the own frame, or a nearer candidate already has the pixel)
                A pixel is blended at most once, and image still holds the own frame's bytes there when it is.  With T = 1 nothing is ever
                blended (dist is 0 or 1 = T); with the gain off as well the call is the existing hard fill.
blend_frame     frame q of a clip: the own frame through the window (id 1), seam_distance of its mask, then every candidate of
                fill.neighbour_order in its order rendered ALONE onto a zeroed layer, overlap_sums -> gains -> blend_layer.

Not here: feathering between two neighbours' regions, multi-band blending, gains smoothed over time or solved jointly over the clip,
vignetting, occlusion tests between candidates, the clip's last frame.
"""
import numpy as np

import stabilize_crop_spec_numpy as crop
import stabilize_fill_spec_numpy as fill

FEATHER_DEFAULT = 16        # pixels of the own frame next to its empty band that are mixed: a choice, not a measurement
FEATHER_MAX = 64
MIN_OVERLAP_DEFAULT = 1024  # overlap pixels below which a candidate gets no gain: a choice, not a measurement
GAIN_MIN = 16384            # 1 / 4
GAIN_ONE = 65536
GAIN_MAX = 262144           # 4


def row_distance(mask, T):
    """h (rows, cols) int64: along the row to the nearest empty pixel, capped at T; 0 on an empty pixel"""
    empty = np.asarray(mask) == 0
    rows, cols = empty.shape
    h = np.where(empty, 0, T).astype(np.int64)
    for d in range(1, T):
        near = np.zeros_like(empty)
        near[:, d:] |= empty[:, :cols - d] if d < cols else False
        near[:, :max(cols - d, 0)] |= empty[:, d:]
        h = np.where(near, np.minimum(h, d), h)
    return h


def seam_distance(mask, T):
    assert 1 <= T <= FEATHER_MAX
    h = row_distance(mask, T)
    rows = h.shape[0]
    d = h.copy()
    for dy in range(1, T):
        if dy >= rows:
            break
        d[dy:] = np.minimum(d[dy:], np.maximum(dy, h[:rows - dy]))
        d[:rows - dy] = np.minimum(d[:rows - dy], np.maximum(dy, h[dy:]))
    return d.astype(np.uint8)


def _planes(a):
    """(rows, cols) or (rows, cols, CH) -> (rows, cols, CH)"""
    a = np.asarray(a)
    return a[..., None] if a.ndim == 2 else a


def overlap_sums(image, source, layer_image, layer_mask):
    img, lay = _planes(image), _planes(layer_image)
    ch = img.shape[2]
    sel = (np.asarray(source) == 1) & (np.asarray(layer_mask) != 0)
    out = np.zeros(8, dtype=np.uint64)
    out[0] = int(sel.sum())
    for c in range(ch):
        out[1 + c] = int(img[..., c][sel].astype(np.int64).sum())
        out[1 + ch + c] = int(lay[..., c][sel].astype(np.int64).sum())
    return out


def gains(sums, ch, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0):
    """-> list of ch Python integers"""
    s = [int(x) for x in sums]
    out = []
    for c in range(ch):
        si, sl = s[1 + c], s[1 + ch + c]
        if gain_mode == 1 or s[0] < min_overlap or sl == 0:
            out.append(GAIN_ONE)
        else:
            out.append(min(max((si * 65536 + (sl >> 1)) // sl, GAIN_MIN), GAIN_MAX))
    return out


def blend_layer(image, mask, source, dist, T, layer_image, layer_mask, source_id, G):
    """image, mask and source are changed IN PLACE.  -> (filled, blended)"""
    assert 2 <= source_id <= 255 and 1 <= T <= FEATHER_MAX
    img, lay = _planes(image), _planes(layer_image)
    on = np.asarray(layer_mask) != 0
    d = np.asarray(dist).astype(np.int64)
    take = on & (source == 0)
    mix = on & (source == 1) & (d < T)
    for c in range(img.shape[2]):
        k = np.minimum(255, (int(G[c]) * lay[..., c].astype(np.int64) + 32768) >> 16)
        own = img[..., c].astype(np.int64)
        new = np.where(take, k, np.where(mix, (d * own + (T - d) * k + (T >> 1)) // T, own))
        img[..., c] = new.astype(np.uint8)
    mask[take] = 1
    source[take | mix] = source_id
    return int(take.sum()), int(mix.sum())


def blend_frame(images, depths, Rs, ts, K, A, c, As, cs, scales, q, M_own, m_own, window, radius=fill.RADIUS_DEFAULT, T=FEATHER_DEFAULT,
                min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, mode=0, q5_mode=0, iterations=0):
    """frame q of a clip through the window, blended.  -> dict(image, mask, source, dist, gains (2 radius, 3; GAIN_ONE where a candidate is
    skipped or a channel unused), sums (2 radius, 8), counts [none, own_untouched, (filled, blended) per offset -1, +1, -2, +2, ...])"""
    npairs = len(depths)
    out = np.zeros_like(np.ascontiguousarray(images[q], dtype=np.uint8))
    rows, cols = out.shape[:2]
    ch = 1 if out.ndim == 2 else out.shape[2]
    mask, source = np.zeros((rows, cols), dtype=np.uint8), np.zeros((rows, cols), dtype=np.uint8)
    G = np.full((2 * radius, 3), GAIN_ONE, dtype=np.uint32)
    S = np.zeros((2 * radius, 8), dtype=np.uint64)
    per = [[0, 0] for _ in range(2 * radius)]
    own = 0
    dist = np.zeros((rows, cols), dtype=np.uint8)
    if window[2] >= 1:
        own = crop.fill_from_window(out, mask, source, images[q], depths[q], Rs[q], ts[q], K, M_own, m_own, 1, window, mode, q5_mode, iterations)
        dist = seam_distance(mask, T)
        for n in (fill.neighbour_order(q, npairs, radius) if radius else []):
            sid = fill.source_id(n - q)
            M, m = fill.neighbour_pose(A, c, As, cs, scales, q, n)
            layer, lmask, lsource = np.zeros_like(out), np.zeros_like(mask), np.zeros_like(mask)
            crop.fill_from_window(layer, lmask, lsource, images[n], depths[n], Rs[n], ts[n], K, M, m, sid, window, mode, q5_mode, iterations)
            S[sid - 2] = overlap_sums(out, source, layer, lmask)
            g = gains(S[sid - 2], ch, min_overlap, gain_mode)
            G[sid - 2, :ch] = g
            per[sid - 2] = list(blend_layer(out, mask, source, dist, T, layer, lmask, sid, g))
    filled, blended = sum(p[0] for p in per), sum(p[1] for p in per)
    counts = [mask.size - own - filled, own - blended] + [x for p in per for x in p]
    return dict(image=out, mask=mask, source=source, dist=dist, gains=G, sums=S, counts=counts)
