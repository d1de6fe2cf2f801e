"""Executable definition of the clean plate (include/rsdsfm_plate.h): the per-pixel, per-channel lower median of the own frame of a solved clip
and its neighbours, each rendered ALONE into the own frame's (virtual) camera, and a per-pixel "this moved" flag from the own frame's distance to
that median over a 3 x 3 patch.  The reference has no counterpart (main.cc:380-523 solves pairs one by one and never relates them); this file is
the definition and the kernel (csrc/plate_kernels.hip) and host functions (csrc/plate_host.hip) reproduce it bit for bit.  Every render is
tests/retime_spec_numpy.py's and tests/stabilize_crop_spec_numpy.py's, the record and the gains tests/stabilize_blend_spec_numpy.py's, the gained
bytes and the 3 x 3 box tests/denoise_spec_numpy.py's, imported and unchanged.

Integers only.  threshold tau 1 .. 255 (default 24, the retimer's conflict threshold: a choice); min_votes 1 .. 15 (default 3: below three
candidates a median outvotes nobody); radius K 1 .. 7 (default 2): at most 14 layers, 15 candidates.

gains        per layer j and channel c G_jc = the denoise's gains(record j); 65536 without a record.  k_jc = min(255, (G_jc L_jc + 32768) >> 16).
candidates   at p: R_c(p) if mR(p) != 0; k_jc(p) for every j with mL_j(p) != 0.  n(p) = their number, 0 .. 15.
plate        n >= 1: P_c(p) = the element at index (n - 1) >> 1 of the ascending order of channel c's candidates (the LOWER median), mask 1;
             n == 0: image 0, mask 0.  votes = n.
moving       v(p) = mR(p) != 0 and n(p) >= min_votes;  e(p) = sum_c |R_c(p) - P_c(p)| where v(p)
             D(p) = sum of e(p') and N(p) = CH #{p'} over the p' of the 3 x 3 window about p inside the frame with v(p')
             flag = 0 where mR == 0; 3 (undecided) where mR != 0 and N == 0; 2 (moving) where D > tau N; 1 (static) otherwise
counts       [unset, static, moving, undecided] = the pixels with flag 0, 1, 2, 3
frame        source 0 (the own frame) through the window with id 1 and its source plane; every other source rendered alone (id 2; through the
             occlusion test or the search when asked), blend.overlap_sums(reference, its source plane, layer) -> record j; one median.

Per channel, so the plate depends on the multiset of candidate values only: the order of the layers and ties change nothing.

Not here: the flag fed back into the denoise, the super-resolution or the fill; a vector (colour-consistent) median; weighted medians; temporal
smoothing or morphology of the flag; inpainting where every source saw the mover.
"""
import numpy as np

import denoise_spec_numpy as denoise
import retime_spec_numpy as retime
import stabilize_blend_spec_numpy as blend
import stabilize_crop_spec_numpy as crop

THRESHOLD_DEFAULT, THRESHOLD_MAX = 24, 255  # a choice, not a measurement
MIN_VOTES_DEFAULT, MIN_VOTES_MAX = 3, 15
RADIUS_DEFAULT, RADIUS_MAX = 2, 7
LAYERS_MAX = 2 * RADIUS_MAX
MIN_OVERLAP_DEFAULT = blend.MIN_OVERLAP_DEFAULT
UNSET = 1 << 16  # above every byte: sorts last

neighbour_order = denoise.neighbour_order


def median(ref, ref_mask, layers, records=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, threshold=THRESHOLD_DEFAULT, min_votes=MIN_VOTES_DEFAULT):
    """layers: a list of 0 .. 14 (image, mask); records: None or one record (or None) per layer
    -> dict(image, mask, votes, moving (rows, cols) uint8, counts [unset, static, moving, undecided])"""
    assert len(layers) <= LAYERS_MAX and 1 <= threshold <= THRESHOLD_MAX and 1 <= min_votes <= MIN_VOTES_MAX
    gray = np.asarray(ref).ndim == 2
    R = denoise._planes(ref).astype(np.int64)
    ch = R.shape[2]
    mR = np.asarray(ref_mask) != 0
    assert mR.shape == R.shape[:2]
    values, valid = [R], [mR]
    for j, (image, mask) in enumerate(layers):
        G = denoise.gains(records[j] if records is not None else None, ch, min_overlap, gain_mode)
        values.append(denoise.gained(image, G))
        valid.append(np.asarray(mask) != 0)
    values, valid = np.stack(values), np.stack(valid)  # (1 + L, rows, cols, CH), (1 + L, rows, cols)
    n = valid.sum(axis=0)
    order = np.sort(np.where(valid[..., None], values, UNSET), axis=0)
    index = np.maximum(n - 1, 0) >> 1
    P = np.take_along_axis(order, np.broadcast_to(index[None, ..., None], (1,) + R.shape), axis=0)[0]
    P = np.where((n > 0)[..., None], P, 0)
    v = mR & (n >= min_votes)
    e = np.where(v, np.abs(R - P).sum(axis=-1), 0)
    D, N = denoise.box3(e), ch * denoise.box3(v.astype(np.int64))
    flag = np.where(~mR, 0, np.where(N == 0, 3, np.where(D > threshold * N, 2, 1))).astype(np.uint8)
    out = P.astype(np.uint8)
    return dict(image=out[..., 0] if gray else out, mask=(n > 0).astype(np.uint8), votes=n.astype(np.uint8), moving=flag,
                counts=[int((flag == k).sum()) for k in range(4)])


def plate_frame(images, depths, Rs, ts, K, M, m, window=None, threshold=THRESHOLD_DEFAULT, min_votes=MIN_VOTES_DEFAULT, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0,
                occlusion=0, search_on=0, tol_q16=0, mode=0, q5_mode=0, iterations=0):
    """images, depths, Rs, ts: 1 .. 15 sources, source 0 the own frame; M (nsrc, 3, 3), m (nsrc, 3): every source's pose in the target camera.
    -> median's dict plus ref (image, mask, source), layers [(image, mask), ...] and records (nsrc - 1, 8) uint64"""
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
    out = median(ref, rmask, layers, list(records), min_overlap, gain_mode, threshold, min_votes)
    return dict(out, ref=(ref, rmask, rsource), layers=layers, records=records)
