"""Executable definition of the clean plate's colour-consistent estimator (include/rsdsfm_plate_medoid.h): the L1 MEDOID of the own frame of a
solved clip and its neighbours in place of tests/plate_spec_numpy.py's per-channel lower median, which may give a plate pixel whose channels
come from different sources -- grey (100, 100, 100), red (0, 0, 255) and blue (255, 0, 0) give (100, 0, 100), a colour no candidate has.  The
reference has no counterpart; this file is the definition and the kernel (csrc/plate_medoid_kernels.hip) and the host functions
(csrc/plate_host.hip) reproduce it bit for bit.  The gains, the candidates, n, the mask, the votes, the flag and the counts are
tests/plate_spec_numpy.py's, and every render is the one its plate_frame makes: imported and unchanged.

Integers only, no division.

gains        plate_spec_numpy's: k_jc = min(255, (G_jc L_jc + 32768) >> 16).
candidates   at p: R(p) if mR(p) != 0; k_j(p) for every j with mL_j(p) != 0.  n(p) = their number, 0 .. 15.
plate        n >= 1: for every valid candidate i  cost_i = sum over the valid j of sum_c |v_ic - v_jc|  (at most 14 * 3 * 255 = 10710),
             colour_i = v_i0 | v_i1 << 8 | v_i2 << 16 (channel 0 least significant: the pixel's little-endian packed dword),
             key_i = (cost_i << 24) | colour_i, and P(p) = the colour of the candidate with the smallest key; mask 1.
             n == 0: image 0, mask 0.  votes = n.
             Two candidates with equal keys have equal colours, so P depends on the multiset of candidate colours only: the order of the layers
             and ties change no byte.
moving       plate_spec_numpy's v, e, D, N, flag and counts, word for word, with this P.
frame        plate_spec_numpy.plate_frame's reference, layers and records; one medoid over them.

Consequences (tests/test_plate_medoid_cpu.py holds the definition to each):
(a) With one channel the medoid is the lower median.  The sum of absolute deviations sum_j |x - x_j| is smallest at every median of the x_j;
    for an odd n that is the middle value (every candidate of that value has the same key), for an even n both middle values tie on cost, and
    the smaller key is the smaller value: the element at index (n - 1) >> 1 of the ascending order.
(b) With three channels whose candidates are all grey (b = g = r) and no gain, the distance of two candidates is 3 |x_i - x_j|, the costs order
    as in (a), the colours order as the values: the medoid is the median's bytes.
(c) With two candidates the costs are equal, and the plate is the candidate with the smaller packed colour -- a whole candidate, not the
    per-channel minimum the median gives.

Not here: weighted medoids; a geometric median that is not a candidate; a plane that says which source was chosen (ambiguous under ties).
"""
import numpy as np

import denoise_spec_numpy as denoise
import plate_spec_numpy as plate

THRESHOLD_DEFAULT, MIN_VOTES_DEFAULT, MIN_OVERLAP_DEFAULT = plate.THRESHOLD_DEFAULT, plate.MIN_VOTES_DEFAULT, plate.MIN_OVERLAP_DEFAULT
NO_KEY = 1 << 62  # a candidate that is not there: above every key (costs stay below 2 ** 14, colours below 2 ** 24)


def candidates(ref, ref_mask, layers, records=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0):
    """-> values (1 + L, rows, cols, CH) int64: the own pixel and the gained layers; valid (1 + L, rows, cols) bool"""
    R = denoise._planes(ref).astype(np.int64)
    ch = R.shape[2]
    mR = np.asarray(ref_mask) != 0
    assert mR.shape == R.shape[:2]
    values, valid = [R], [mR]
    for j, (image, mask) in enumerate(layers):
        G = denoise.gains(records[j] if records is not None else None, ch, min_overlap, gain_mode)
        values.append(denoise.gained(image, G).astype(np.int64))
        valid.append(np.asarray(mask) != 0)
    return np.stack(values), np.stack(valid)


def medoid(ref, ref_mask, layers, records=None, min_overlap=MIN_OVERLAP_DEFAULT, gain_mode=0, threshold=THRESHOLD_DEFAULT, min_votes=MIN_VOTES_DEFAULT):
    """layers: a list of 0 .. 14 (image, mask); records: None or one record (or None) per layer
    -> dict(image, mask, votes, moving (rows, cols) uint8, counts [unset, static, moving, undecided]), as plate_spec_numpy.median"""
    assert len(layers) <= plate.LAYERS_MAX and 1 <= threshold <= plate.THRESHOLD_MAX and 1 <= min_votes <= plate.MIN_VOTES_MAX
    gray = np.asarray(ref).ndim == 2
    values, valid = candidates(ref, ref_mask, layers, records, min_overlap, gain_mode)
    R, mR = values[0], valid[0]
    ch = R.shape[2]
    n = valid.sum(axis=0)
    colour = sum(values[..., c] << (8 * c) for c in range(ch))
    best = np.full(n.shape, NO_KEY, dtype=np.int64)
    for i in range(len(values)):
        cost = np.where(valid, np.abs(values[i][None] - values).sum(axis=-1), 0).sum(axis=0)
        assert cost.max() <= 14 * 255 * ch
        best = np.minimum(best, np.where(valid[i], (cost << 24) | colour[i], NO_KEY))
    P = np.stack([(best >> (8 * c)) & 0xff for c in range(ch)], axis=-1)
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
    """plate_spec_numpy.plate_frame with its median replaced by the medoid over the reference, the layers and the records it returns
    -> medoid's dict plus ref, layers and records"""
    r = plate.plate_frame(images, depths, Rs, ts, K, M, m, window, threshold, min_votes, min_overlap, gain_mode, occlusion, search_on, tol_q16, mode, q5_mode, iterations)
    ref, rmask, _ = r["ref"]
    out = medoid(ref, rmask, r["layers"], list(r["records"]), min_overlap, gain_mode, threshold, min_votes)
    return dict(out, ref=r["ref"], layers=r["layers"], records=r["records"])


def spec_of(case):
    """the medoid of a case of plate_cases (random_case, constructed, make_golden_plate.median_cases)"""
    return medoid(case["ref"], case["rmask"], case["layers"], None if case["records"] is None else list(case["records"]), case["min_overlap"] or MIN_OVERLAP_DEFAULT,
                  case["gain_mode"], case["threshold"], case["min_votes"])


def run_spec(case, q=None):
    """the definition on frame q of a case of plate_cases.all_cases, as plate_cases.run_spec.  -> plate_frame's dict plus sources"""
    import denoise_cases as dcases

    src, M, m = dcases.sources_and_poses(case, q)
    pick = lambda k: [case[k][n] for n in src]
    r = plate_frame(pick("frames"), pick("depths"), pick("Rs"), pick("ts"), case["K"], M, m, case["window"], case["threshold"], case["min_votes"], case["min_overlap"],
                    case["gain_mode"], case["occlusion"], case["search"], case["tol_q16"], case["mode"], case["q5_mode"], case["iterations"])
    return dict(r, sources=src)
