"""The link between consecutive pairs of a clip, the chain of scales and poses and the clip's points (include/rsdsfm_trajectory.h), defined
in float64 numpy: the kernels of csrc/link_kernels.hip reproduce the link and the points bit for bit, csrc/link_host.hip the chain to the
last digits of exp / sin / cos.  Every operation is rounded once and none is fused (the library is built with -ffp-contract=off).

A differential solve fixes its scale per pair: pair p's v and depth map are in one unit, pair p + 1's in another.  The link measures the
ratio of the two units from the pixels both pairs gave a depth to.

F is the field pair p was solved on (rows x cols x 2, (fu, fv) per pixel), Z_p and Z_n the depth maps of pairs p and p + 1 ((rows, cols)
here; column-major on the device), (v, w, k) pair p's final motion, K = (fx, fy, cx, cy).  A depth is VALID iff it is finite and > 0.
For pixel (row i, column j) with z = Z_p[i, j] valid:
    1  flatten_point's expressions (csrc/device_math.hpp):  qx = (j - cx) * 1.0 / fx,  qy = (i - cy) * 1.0 / fy,
       alpha = 1 + gamma * fv / rows  (1 in global-shutter mode),  part1 = gamma * i / rows,  part2 = 1.0 + gamma * (i + fv) / rows,
       alpha_k = 0.5 * (part2 * part2 - part1 * part1)
    2  beta = (2.0 * (alpha + k * alpha_k)) / (2.0 + k),  b = beta / gamma
    3  z_pred = z * (1.0 + b * (w0 * qy - w1 * qx)) + b * v2      (the z of P' = P + b (v + w x P), P = z (qx, qy, 1))
    4  r2 = floor((i + fv) + 0.5),  c2 = floor((j + fu) + 0.5);  INSIDE iff 0 <= r2 <= rows - 1 and 0 <= c2 <= cols - 1 (false for NaN)
    5  z2 = Z_n[r2, c2];  ratio = z2 / z_pred
    6  the pixel is a CORRESPONDENCE iff inside, z2 valid, z_pred finite and > 0, and ratio finite and > 0 (a quotient that overflows or
       underflows to zero is none: the plane keeps 0 for "no correspondence")
    7  plane[i, j] = the bit pattern of ratio (uint64) for a correspondence, else 0
Per link: n = the number of correspondences; ratio = their LOWER median, the element of rank (n - 1) // 2 in sorted order (one of the
inputs, no averaging; NaN for n = 0); agree = the number of correspondences r with r <= ratio * (1.0 + tol) and r * (1.0 + tol) >= ratio
(0 for n = 0); valid = n >= min_links.
"""
import numpy as np

TOL_DEFAULT, MIN_LINKS_DEFAULT = 0.1, 16


def point_terms(F, K, gamma, k, global_shutter=False):
    """steps 1 - 2 for every pixel: (qx, qy, b), each (rows, cols)"""
    F = np.asarray(F, dtype=np.float64)
    rows, cols = F.shape[:2]
    fx, fy, cx, cy = (np.float64(x) for x in K)
    gamma, k, h = np.float64(gamma), np.float64(k), np.float64(rows)
    ii, jj = np.mgrid[0:rows, 0:cols].astype(np.float64)
    fv = F[..., 1]
    qx = (jj - cx) * 1.0 / fx
    qy = (ii - cy) * 1.0 / fy
    alpha = np.ones((rows, cols)) if global_shutter else 1 + gamma * fv / h
    part1 = gamma * ii / h
    part2 = 1.0 + gamma * (ii + fv) / h
    alpha_k = 0.5 * (part2 * part2 - part1 * part1)
    beta = (2.0 * (alpha + k * alpha_k)) / (2.0 + k)
    return qx, qy, beta / gamma


def valid_depth(z):
    with np.errstate(invalid="ignore"):
        return np.isfinite(z) & (z > 0.0)


def predict(F, Z_p, v, w, k, K, gamma, global_shutter=False):
    """steps 1 - 4: (z_pred, r2, c2, inside) per pixel; r2 / c2 are int64 and 0 where the landing pixel is not inside"""
    F, Z_p = np.asarray(F, dtype=np.float64), np.asarray(Z_p, dtype=np.float64)
    rows, cols = Z_p.shape
    assert F.shape == (rows, cols, 2)
    v, w = np.asarray(v, dtype=np.float64), np.asarray(w, dtype=np.float64)
    ii, jj = np.mgrid[0:rows, 0:cols].astype(np.float64)
    with np.errstate(all="ignore"):
        qx, qy, b = point_terms(F, K, gamma, k, global_shutter)
        z_pred = Z_p * (1.0 + b * (w[0] * qy - w[1] * qx)) + b * v[2]
        r2 = np.floor((ii + F[..., 1]) + 0.5)
        c2 = np.floor((jj + F[..., 0]) + 0.5)
        inside = (r2 >= 0.0) & (r2 <= rows - 1.0) & (c2 >= 0.0) & (c2 <= cols - 1.0)
    r2 = np.where(inside, r2, 0.0).astype(np.int64)
    c2 = np.where(inside, c2, 0.0).astype(np.int64)
    return z_pred, r2, c2, inside


def ratio_plane(F, Z_p, v, w, k, Z_n, K, gamma, global_shutter=False):
    """steps 1 - 7: the (rows, cols) uint64 plane"""
    Z_p, Z_n = np.asarray(Z_p, dtype=np.float64), np.asarray(Z_n, dtype=np.float64)
    assert Z_p.shape == Z_n.shape
    z_pred, r2, c2, inside = predict(F, Z_p, v, w, k, K, gamma, global_shutter)
    z2 = Z_n[r2, c2]
    with np.errstate(all="ignore"):
        ratio = z2 / z_pred
        ok = valid_depth(Z_p) & inside & valid_depth(z2) & valid_depth(z_pred) & valid_depth(ratio)
    return np.where(ok, np.ascontiguousarray(ratio).view(np.uint64), np.uint64(0))


def link_record(plane, tol=TOL_DEFAULT, min_links=MIN_LINKS_DEFAULT):
    """the per-link record of a plane: dict(n, ratio, agree, valid)"""
    bits = np.asarray(plane, dtype=np.uint64).ravel()
    r = np.sort(bits[bits != 0].view(np.float64))  # positive finite doubles order as their bit patterns
    n = int(r.size)
    if n == 0:
        return dict(n=0, ratio=float("nan"), agree=0, valid=bool(0 >= min_links))
    med = r[(n - 1) // 2]
    onetol = np.float64(1.0) + np.float64(tol)
    agree = int(np.count_nonzero((r <= med * onetol) & (r * onetol >= med)))
    return dict(n=n, ratio=float(med), agree=agree, valid=bool(n >= min_links))


def link(F, Z_p, v, w, k, Z_n, K, gamma, global_shutter=False, tol=TOL_DEFAULT, min_links=MIN_LINKS_DEFAULT):
    plane = ratio_plane(F, Z_p, v, w, k, Z_n, K, gamma, global_shutter)
    return dict(link_record(plane, tol, min_links), plane=plane)


def rodrigues(a):
    """exp([a]x) = I + sin(t) / t [a]x + (1 - cos(t)) / t^2 [a]x^2, t = |a|; the series' first terms below t = 1e-8"""
    a = np.asarray(a, dtype=np.float64)
    t2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
    t = np.sqrt(t2)
    if t < 1e-8:
        s, c = 1.0 - t2 / 6.0, 0.5 - t2 / 24.0
    else:
        s, c = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    X = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + s * X + c * (X @ X)


def chain(ratios, valids, vs, ws, gamma):
    """The clip's scales and poses.  ratios / valids: the F - 2 links; vs / ws: the F - 1 pairs' motions.
    S_0 = 1, S_{q+1} = S_q / ratio_q (S_q where link q is not valid: broken[q] = 1).  Frame q's first scanline in frame 0's coordinates:
    A_0 = I, c_0 = 0, R_q = exp([w_q / gamma]x), A_{q+1} = A_q R_q^T, c_{q+1} = c_q - A_{q+1} (S_q v_q / gamma).
    -> dict(scales (F - 1), A (F, 3, 3), c (F, 3), broken (F - 2) uint8)"""
    vs, ws = np.asarray(vs, dtype=np.float64).reshape(-1, 3), np.asarray(ws, dtype=np.float64).reshape(-1, 3)
    npairs = vs.shape[0]
    assert ws.shape[0] == npairs and len(ratios) == len(valids) == max(npairs - 1, 0)
    gamma = np.float64(gamma)
    scales, broken = np.ones(npairs), np.zeros(max(npairs - 1, 0), dtype=np.uint8)
    for q in range(npairs - 1):
        good = bool(valids[q]) and np.isfinite(ratios[q]) and ratios[q] > 0.0
        scales[q + 1] = scales[q] / ratios[q] if good else scales[q]
        broken[q] = 0 if good else 1
    A, c = np.zeros((npairs + 1, 3, 3)), np.zeros((npairs + 1, 3))
    A[0] = np.eye(3)
    for q in range(npairs):
        A[q + 1] = A[q] @ rodrigues(ws[q] / gamma).T
        c[q + 1] = c[q] - A[q + 1] @ (scales[q] * vs[q] / gamma)
    return dict(scales=scales, A=A, c=c, broken=broken)


def clip_points(X, scale, A, c):
    """pair q's world points (rows, cols, 3) float32 in frame q's coordinates -> the clip's: A (scale * X) + c in float64, terms in column
    order, rounded once to float32; a point that is exactly (0, 0, 0) stays (0, 0, 0)"""
    X = np.asarray(X, dtype=np.float32)
    A, c, s = np.asarray(A, dtype=np.float64).reshape(3, 3), np.asarray(c, dtype=np.float64).reshape(3), np.float64(scale)
    x = X.astype(np.float64)
    p0, p1, p2 = s * x[..., 0], s * x[..., 1], s * x[..., 2]
    with np.errstate(all="ignore"):
        out = np.stack([((A[i, 0] * p0 + A[i, 1] * p1) + A[i, 2] * p2) + c[i] for i in range(3)], axis=-1).astype(np.float32)
    zero = (X[..., 0] == 0) & (X[..., 1] == 0) & (X[..., 2] == 0)
    return np.where(zero[..., None], np.float32(0), out)
