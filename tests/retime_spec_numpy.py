"""Executable definition of the retimer (include/rsdsfm_retime.h): a frame of a solved clip at ANY instant along the camera path, rendered from
the two input frames next to it in time and merged by how near each is.  The reference has no counterpart (main.cc:380-523 solves pairs one
by one and never relates them); this file is the definition and the kernel (csrc/retime_kernels.hip) and host functions
(csrc/retime_host.hip, compiled with -ffp-contract=off) reproduce it -- the merge and the frame call bit for bit.
tests/stabilize_crop_spec_numpy.py, tests/stabilize_visible_spec_numpy.py, tests/stabilize_search_spec_numpy.py,
tests/stabilize_spec_numpy.py and tests/link_spec_numpy.py are imported and unchanged.

The poses are float64 with one rounding per operation, sums taken in the order written; the merge is integer arithmetic only.

path_at        q = floor(t), tau = t - q.  tau == 0: entry q, bit for bit.  Else A_t = A_q rodrigues(tau so3_log(A_q^T A_{q+1})) (the path
               smoother's logarithm and exponential), c_t = c_q + tau (c_{q+1} - c_q): piecewise geodesic, no spline.
retime_poses   the sources n0 = floor(t) and, when tau > 0, n0 + 1; for each M = A_t^T A_n, m = (A_t^T (c_n - c_t)) / S_n (the border fill's
               neighbour_pose); weight 0 with one source, else rint(tau 65536) clamped to [1, 65535].
merge          per pixel, a = mask_a != 0, b = mask_b != 0, d = max over the channels of |a_c - b_c|:
                 neither                          image 0, mask 0, source 0
                 a only                           a's bytes, mask 1, source 1
                 b only                           b's bytes, mask 1, source 2
                 both, d <= threshold             (a_c (65536 - w) + b_c w + 32768) >> 16, mask 1, source 3
                 both, d > threshold, w <= 32768  a's bytes, mask 1, source 4
                 both, d > threshold, w > 32768   b's bytes, mask 1, source 5
               counts = [none, a only, b only, dissolved, conflict].
retime_frame   every source rendered ALONE onto zeroed planes (crop.fill_from_window; occlusion: visible.fill_from_visible; occlusion and
               search: search.fill_from_search), then merge.

Not here: splines through the poses, filling from further neighbours, inpainting, an exposure gain between the two sources.
"""
import numpy as np

import link_spec_numpy as link
import stabilize_crop_spec_numpy as crop
import stabilize_search_spec_numpy as search
import stabilize_spec_numpy as stab
import stabilize_visible_spec_numpy as visible

NONE, FROM_A, FROM_B, DISSOLVED, CONFLICT_A, CONFLICT_B = range(6)
THRESHOLD_DEFAULT = 24  # a choice, not a measurement
WEIGHT_ONE = 65536


def path_at(A_path, c_path, t):
    """A_path (F, 3, 3), c_path (F, 3), t in [0, F - 1] -> (A_t (3, 3), c_t (3,))"""
    A = np.asarray(A_path, dtype=np.float64).reshape(-1, 3, 3)
    c = np.asarray(c_path, dtype=np.float64).reshape(-1, 3)
    t = np.float64(t)
    assert np.isfinite(t) and 0 <= t <= A.shape[0] - 1 and c.shape[0] == A.shape[0]
    q = int(np.floor(t))
    tau = t - np.floor(t)
    if tau == 0:
        return A[q].copy(), c[q].copy()
    step = tau * stab.so3_log(stab._mat3(A[q].T, A[q + 1]))
    return stab._mat3(A[q], link.rodrigues(step)), c[q] + tau * (c[q + 1] - c[q])


def weight_q16(tau):
    """0 for tau == 0, else rint(tau 65536) clamped to [1, 65535]"""
    tau = np.float64(tau)
    return 0 if tau == 0 else int(min(max(np.rint(tau * 65536.0), 1), WEIGHT_ONE - 1))


def retime_poses(A, c, A_path, c_path, scales, nsources, t):
    """-> dict(sources (n0,) or (n0, n0 + 1), weight, M (nsrc, 3, 3), m (nsrc, 3), A_t, c_t)"""
    A = np.asarray(A, dtype=np.float64).reshape(-1, 3, 3)
    c = np.asarray(c, dtype=np.float64).reshape(-1, 3)
    S = np.asarray(scales, dtype=np.float64).reshape(-1)
    t = np.float64(t)
    assert nsources >= 1 and np.isfinite(t) and 0 <= t <= nsources - 1
    n0 = int(np.floor(t))
    tau = t - np.floor(t)
    sources = (n0,) if tau == 0 else (n0, n0 + 1)
    A_t, c_t = path_at(np.asarray(A_path, dtype=np.float64).reshape(-1, 3, 3)[:nsources], np.asarray(c_path, dtype=np.float64).reshape(-1, 3)[:nsources], t)
    M, m = [], []
    for n in sources:
        assert np.isfinite(S[n]) and S[n] > 0
        M.append(stab._mat3(A_t.T, A[n]))
        m.append(stab._matvec(A_t.T, c[n] - c_t) / S[n])
    return dict(sources=sources, weight=weight_q16(tau), M=np.array(M), m=np.array(m), A_t=A_t, c_t=c_t)


def merge(image_a, mask_a, image_b=None, mask_b=None, weight=0, threshold=THRESHOLD_DEFAULT):
    """image (rows, cols) or (rows, cols, 3) uint8, mask (rows, cols) uint8 (0 = empty); b None: absent everywhere (weight 0).
    -> dict(image, mask, source (rows, cols) uint8, counts [none, a only, b only, dissolved, conflict])"""
    ia = np.ascontiguousarray(image_a, dtype=np.uint8)
    a = np.asarray(mask_a) != 0
    assert (image_b is None) == (mask_b is None) and 0 <= weight < WEIGHT_ONE and 0 <= threshold <= 255
    if image_b is None:
        assert weight == 0
        ib, b = np.zeros_like(ia), np.zeros_like(a)
    else:
        ib, b = np.ascontiguousarray(image_b, dtype=np.uint8), np.asarray(mask_b) != 0
    assert ia.shape == ib.shape and a.shape == b.shape == ia.shape[:2]
    va, vb = ia.reshape(a.shape + (-1,)).astype(np.int64), ib.reshape(a.shape + (-1,)).astype(np.int64)
    d = np.abs(va - vb).max(axis=-1)
    both = a & b
    source = np.zeros(a.shape, dtype=np.uint8)
    source[a & ~b] = FROM_A
    source[b & ~a] = FROM_B
    source[both & (d <= threshold)] = DISSOLVED
    source[both & (d > threshold)] = CONFLICT_A if weight <= 32768 else CONFLICT_B
    mix = (va * (WEIGHT_ONE - weight) + vb * weight + 32768) >> 16
    s = source[..., None]
    out = np.where(s == DISSOLVED, mix, np.where((s == FROM_A) | (s == CONFLICT_A), va, np.where(s == NONE, 0, vb)))
    bins = np.bincount(source.reshape(-1), minlength=6)
    counts = [int(bins[0]), int(bins[1]), int(bins[2]), int(bins[3]), int(bins[4] + bins[5])]
    return dict(image=out.astype(np.uint8).reshape(ia.shape), mask=(a | b).astype(np.uint8), source=source, counts=counts)


def render_layer(image, depth, R, t, K, M, m, window, source_id=1, occlusion=0, search_on=0, tol_q16=0, mode=0, q5_mode=0, iterations=0):
    """one source alone on zeroed planes -> (image, mask)"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    rows, cols = np.asarray(depth).shape
    out, mask, source = np.zeros_like(image), np.zeros((rows, cols), dtype=np.uint8), np.zeros((rows, cols), dtype=np.uint8)
    if occlusion and search_on:
        search.fill_from_search(out, mask, source, image, depth, R, t, K, M, m, source_id, window, tol_q16, mode, q5_mode, iterations)
    elif occlusion:
        visible.fill_from_visible(out, mask, source, image, depth, R, t, K, M, m, source_id, window, tol_q16, mode, q5_mode, iterations)
    else:
        crop.fill_from_window(out, mask, source, image, depth, R, t, K, M, m, source_id, window, mode, q5_mode, iterations)
    return out, mask


def retime_frame(images, depths, Rs, ts, K, M, m, weight, window=None, threshold=THRESHOLD_DEFAULT, occlusion=0, search_on=0, tol_q16=0, mode=0, q5_mode=0,
                 iterations=0):
    """images, depths, Rs, ts: one or two sources; M (nsrc, 3, 3), m (nsrc, 3), weight: retime_poses'.
    -> merge's dict plus layers [(image, mask), ...]"""
    nsrc = len(images)
    assert nsrc in (1, 2) and (nsrc == 2 or weight == 0)
    rows, cols = np.asarray(depths[0]).shape
    window = (0, 0, rows, cols) if window is None else tuple(window)
    M, m = np.asarray(M, dtype=np.float64).reshape(-1, 3, 3), np.asarray(m, dtype=np.float64).reshape(-1, 3)
    layers = [render_layer(images[k], depths[k], Rs[k], ts[k], K, M[k], m[k], window, FROM_A + k, occlusion, search_on, tol_q16, mode, q5_mode, iterations)
              for k in range(nsrc)]
    b = layers[1] if nsrc == 2 else (None, None)
    return dict(merge(layers[0][0], layers[0][1], b[0], b[1], weight, threshold), layers=layers)
