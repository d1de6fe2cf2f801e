"""Executable definition of the sharpness transfer PER SCANLINE BAND (include/rsdsfm_deblur.h, "per scanline band"): the rows of a rolling-shutter
frame are exposed one after another, so the shake that blurs a hand-held frame changes during the read-out and the frame is typically sharp in
one part and smeared in another.  One tau per neighbour (tests/deblur_spec_numpy.py) is then 0 for the whole frame or a diluted value
everywhere; here every band of rows has its own sharpness record and its own tau, and a row's tau is interpolated between band centres.  This
file imports tests/deblur_spec_numpy.py unchanged and repeats none of it; the kernels (csrc/deblur_bands_kernels.hip) and host functions
(csrc/deblur_host.hip) reproduce it bit for bit.  Integers only.

bands        band_rows = H, a multiple of 16 in [16, 16384] (a 16-row tile then lies in one band); NB = ceil(rows / H) <= BANDS_MAX = 64;
             band(y) = y // H; the last band may be short
band records (NB, 4) uint64, T_b = [pairs, A_R, A_L, 0]: the pairs of deblur_spec_numpy.sharpness, every pair (p, q) in the band of p, its left
             or upper pixel -- a vertical pair across a band border belongs to the upper band.  sum_b T_b is the whole-frame record, exactly
band tau     tau_b = deblur_spec_numpy.tau(T_b, margin, min_pairs): the frame-wide rule applied to the band; no new knob
row tau      centres c_b = b H + H // 2 (also for a short last band); tau(y) = tau_0 for y < c_0, tau_{NB-1} for y >= c_{NB-1}, else with
             b = (y - H // 2) // H and f = (y - H // 2) - b H: tau(y) = (tau_b (H - f) + tau_{b+1} f + H // 2) // H, an integer in 0 .. 32
step         deblur_spec_numpy.step with u(p) = (w(p) tau(row of p) + 8) >> 4; the gate, the gains, the cells, the resolve, the weight plane and
             the counters as they are; u <= 32 per layer, so n <= 240, s <= 61 200 and the limit of 7 layers hold unchanged

Consequences: NB = 1 -> the unbanded accumulate's bytes; every tau_b = 0 -> the own frame's bytes; the order of the layers changes no byte; a
row both of whose surrounding bands have tau = 0 keeps its bytes.

The band height's default (0: off) and the linear interpolation are choices, not measurements.

Not here: band heights that are no multiple of the tile's 16 rows, bands along the columns, a smoother interpolation than the linear one.
"""
import numpy as np

import deblur_spec_numpy as spec
import denoise_spec_numpy as dn

BANDS_MAX = 64
BAND_ROWS_STEP, BAND_ROWS_MAX = 16, 16384


def nbands(rows, band_rows):
    assert band_rows % BAND_ROWS_STEP == 0 and BAND_ROWS_STEP <= band_rows <= BAND_ROWS_MAX
    nb = -(-rows // band_rows)
    assert nb <= BANDS_MAX
    return nb


def band_sharpness(ref, ref_mask, layer, layer_mask, band_rows, record=None, min_overlap=spec.MIN_OVERLAP_DEFAULT, gain_mode=0):
    """-> (NB, 4) uint64, a record per band; a pair counts in the band of its left or upper pixel"""
    ch = dn._planes(ref).shape[2]
    v, YR, YL, _ = spec.lumas(ref, ref_mask, layer, layer_mask, dn.gains(record, ch, min_overlap, gain_mode))
    rows = v.shape[0]
    nb = nbands(rows, band_rows)
    out = np.zeros((nb, 4), dtype=np.uint64)
    for sl_p, sl_q in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))), ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
        both = v[sl_p] & v[sl_q]
        d_r = ((YR[sl_p] - YR[sl_q]) ** 2) * both
        d_l = ((YL[sl_p] - YL[sl_q]) ** 2) * both
        for b in range(nb):
            rows_b = slice(b * band_rows, min((b + 1) * band_rows, both.shape[0]))  # the rows of p
            out[b, 0] += np.uint64(int(both[rows_b].sum()))
            out[b, 1] += np.uint64(int(d_r[rows_b].sum()))
            out[b, 2] += np.uint64(int(d_l[rows_b].sum()))
    return out


def band_taus(records, margin=spec.MARGIN_DEFAULT, min_pairs=spec.MIN_PAIRS_DEFAULT):
    """-> list of NB taus: the frame-wide rule on every band's record"""
    return [spec.tau(T, margin, min_pairs) for T in np.asarray(records, dtype=np.uint64).reshape(-1, 4)]


def row_taus(taus, band_rows, rows):
    """-> (rows,) int64: the band taus interpolated between the band centres"""
    taus = np.asarray(taus, dtype=np.int64)
    nb, H = nbands(rows, band_rows), int(band_rows)
    assert taus.shape == (nb,) and taus.min() >= 0 and taus.max() <= spec.TAU_MAX
    y = np.arange(rows, dtype=np.int64)
    b = np.clip((y - H // 2) // H, 0, max(nb - 2, 0))
    f = (y - H // 2) - b * H
    mid = (taus[b] * (H - f) + taus[np.minimum(b + 1, nb - 1)] * f + H // 2) // H
    return np.where(y < H // 2, taus[0], np.where(y >= (nb - 1) * H + H // 2, taus[nb - 1], mid))


def step(cells, ref, ref_mask, layer, layer_mask, first, t_rows=None, record=None, min_overlap=spec.MIN_OVERLAP_DEFAULT, gain_mode=0,
         strength=spec.STRENGTH_DEFAULT, gate_mode=0):
    """deblur_spec_numpy.step with a factor per row: t_rows (rows,) -> the new cells (a new array)"""
    if layer is None:
        return spec.step(cells, ref, ref_mask, None, None, first, 0, record, min_overlap, gain_mode, strength, gate_mode)
    # u = (w t + 8) >> 4 depends on the row through t alone, so the rows with the factor t are deblur_spec_numpy.step(t)'s rows
    t_rows = np.asarray(t_rows, dtype=np.int64)
    assert t_rows.shape == (np.asarray(ref_mask).shape[0],)
    out = None
    for t in np.unique(t_rows):
        part = spec.step(cells, ref, ref_mask, layer, layer_mask, first, int(t), record, min_overlap, gain_mode, strength, gate_mode)
        out = part.copy() if out is None else out
        out[t_rows == t] = part[t_rows == t]
    return out


def deblur(ref, ref_mask, layers, band_rows, records=None, band_records=None, min_overlap=spec.MIN_OVERLAP_DEFAULT, gain_mode=0, strength=spec.STRENGTH_DEFAULT,
           margin=spec.MARGIN_DEFAULT, min_pairs=spec.MIN_PAIRS_DEFAULT, gate_mode=0):
    """deblur_spec_numpy.deblur with band records: band_records None (computed) or one (NB, 4) array per layer
    -> the resolve dict plus cells (after every step), band_records (n, NB, 4) uint64, band_taus (n lists), row_taus (n arrays)"""
    assert len(layers) <= spec.LAYERS_MAX
    rows = np.asarray(ref_mask).shape[0]
    nb = nbands(rows, band_rows)
    rec = lambda j: records[j] if records is not None else None
    if band_records is None:
        band_records = [band_sharpness(ref, ref_mask, li, lm, band_rows, rec(j), min_overlap, gain_mode) for j, (li, lm) in enumerate(layers)]
    btaus = [band_taus(T, margin, min_pairs) for T in band_records]
    rtaus = [row_taus(t, band_rows, rows) for t in btaus]
    cells, trail = None, []
    for j, (image, mask) in enumerate(list(layers) if layers else [(None, None)]):
        cells = step(cells, ref, ref_mask, image, mask, j == 0, rtaus[j] if layers else None, rec(j) if layers else None, min_overlap, gain_mode, strength, gate_mode)
        trail.append(cells)
    return dict(dn.resolve(cells, np.asarray(ref).ndim == 2), cells=trail, band_records=np.array(band_records, dtype=np.uint64).reshape(-1, nb, 4), band_taus=btaus,
                row_taus=rtaus)


def deblur_frame(images, depths, Rs, ts, K, M, m, band_rows, window=None, strength=spec.STRENGTH_DEFAULT, margin=spec.MARGIN_DEFAULT, min_pairs=spec.MIN_PAIRS_DEFAULT,
                 gate_mode=0, min_overlap=spec.MIN_OVERLAP_DEFAULT, gain_mode=0, **render):
    """deblur_spec_numpy.deblur_frame's renders and overlap records (taken from it, with its arguments) under the banded transfer
    -> deblur's dict plus ref, layers and records"""
    base = spec.deblur_frame(images, depths, Rs, ts, K, M, m, window, strength, margin, min_pairs, gate_mode, min_overlap, gain_mode, **render)
    ref, rmask, _ = base["ref"]
    out = deblur(ref, rmask, base["layers"], band_rows, list(base["records"]), None, min_overlap, gain_mode, strength, margin, min_pairs, gate_mode)
    return dict(out, ref=base["ref"], layers=base["layers"], records=base["records"])


def box_blur_rows(frame, widths):
    """deblur_spec_numpy.box_blur with a width per row (rows odd widths): the varying smear of a rolling-shutter exposure; synth.render_sequence's
    blur with a sequence entry"""
    a = np.asarray(frame)
    widths = np.asarray(widths, dtype=np.int64)
    assert widths.shape == (a.shape[0],)
    out = np.ascontiguousarray(a, dtype=np.uint8).copy()
    for w in np.unique(widths):
        out[widths == w] = spec.box_blur(a, int(w))[widths == w]
    return out
