"""Executable definition of the stabiliser (include/rsdsfm_stabilize.h): a smoothed camera path from the chain's poses, the rigid
transform from every frame's first scanline to its virtual camera on that path, and the dense rectifier with that transform inside its
stage B.  The reference has no counterpart (main.cc:380-523 solves pairs one by one and never relates them); this file is the definition
and the kernels (csrc/stabilize_kernels.hip, compiled with -ffp-contract=off) and host functions (csrc/stabilize_host.hip) reproduce it --
the frame call bit for bit.  tests/rectify_dense_spec_numpy.py and tests/link_spec_numpy.py are imported and unchanged.

All arithmetic is float64 with one rounding per operation; sums are taken in the order written.

so3_log(R)        a = 1/2 (R21 - R12, R02 - R20, R10 - R01), s = sqrt((a0^2 + a1^2) + a2^2), c = 1/2 (((R00 + R11) + R22) - 1),
                  theta = atan2(s, c); a if s < 1e-8, else a (theta / s).  A relative rotation near pi inside one window is
                  ill-conditioned: unsupported, not detected.
smooth_path       one tangent-space mean step about A_q with Gaussian weights g_j = exp(-(j j) / (2 sigma^2)), j = -r .. r ascending,
                  frames outside the clip skipped:  A~_q = A_q rodrigues(sum g so3_log(A_q^T A_{q+j}) / sum g),
                  c~_q = c_q + sum g (c_{q+j} - c_q) / sum g.  A camera that does not move keeps its path exactly.
virtual_poses     M_q = A~_q^T A_q, m_q = (A~_q^T (c_q - c~_q)) / S_q (pair q's own unit): a point X in frame q's first-scanline
                  coordinates is M_q X + m_q in virtual camera q's.
forward_map       the dense spec's stage B up to pg (the point in the first scanline's coordinates), then
                  pv_i = ((M[3i] pg0 + M[3i+1] pg1) + M[3i+2] pg2) + m_i, gx = pv0 / pv2 fx + cx, gy = pv1 / pv2 fy' + cy; D float32.
stabilize_frame   fill_depth, this forward_map, the dense spec's backward_warp.

There is no zoom or crop: with a zoom inside D the fixed point p <- g - D(p) contracts by |zoom - 1| per step and does not converge at
zoom 2.  Cropping is the caller's, guided by the mask and the valid count.
"""
import numpy as np

import link_spec_numpy as link
import rectify_dense_spec_numpy as dense

SIGMA_DEFAULT = 4.0  # frames: a choice, not a measurement


def _mat3(a, b):
    """a @ b for 3 x 3, every entry ((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j)"""
    return np.array([[(a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j] for j in range(3)] for i in range(3)])


def _matvec(a, x):
    return np.array([(a[i, 0] * x[0] + a[i, 1] * x[1]) + a[i, 2] * x[2] for i in range(3)])


def so3_log(R):
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    a = np.array([0.5 * (R[2, 1] - R[1, 2]), 0.5 * (R[0, 2] - R[2, 0]), 0.5 * (R[1, 0] - R[0, 1])])
    s = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    c = 0.5 * (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0)
    theta = np.arctan2(s, c)
    if s < 1e-8:
        return a
    return a * (theta / s)


def smooth_path(A, c, sigma=SIGMA_DEFAULT, radius=0, translation=True):
    """A (F, 3, 3), c (F, 3) from link_spec_numpy.chain -> (A~ (F, 3, 3), c~ (F, 3))"""
    A = np.asarray(A, dtype=np.float64).reshape(-1, 3, 3)
    c = np.asarray(c, dtype=np.float64).reshape(-1, 3)
    F = A.shape[0]
    assert c.shape[0] == F and F >= 1 and np.isfinite(sigma) and sigma > 0 and 0 <= radius <= 1024
    sigma = np.float64(sigma)
    r = int(radius) if radius else int(np.ceil(3.0 * sigma))
    As, cs = np.empty_like(A), np.empty_like(c)
    for q in range(F):
        num, numc, den = np.zeros(3), np.zeros(3), np.float64(0.0)
        At = A[q].T
        for j in range(-r, r + 1):
            if q + j < 0 or q + j > F - 1:
                continue
            g = np.exp(-np.float64(j * j) / (2.0 * sigma * sigma))
            num = num + g * so3_log(_mat3(At, A[q + j]))
            numc = numc + g * (c[q + j] - c[q])
            den = den + g
        As[q] = _mat3(A[q], link.rodrigues(num / den))
        cs[q] = c[q] + numc / den if translation else c[q]
    return As, cs


def virtual_poses(A, c, As, cs, scales, translation=True):
    """-> M (F - 1, 3, 3), m (F - 1, 3): frame q's first-scanline coordinates to virtual camera q's, in pair q's own unit"""
    A, As = np.asarray(A, dtype=np.float64).reshape(-1, 3, 3), np.asarray(As, dtype=np.float64).reshape(-1, 3, 3)
    c, cs = np.asarray(c, dtype=np.float64).reshape(-1, 3), np.asarray(cs, dtype=np.float64).reshape(-1, 3)
    n = A.shape[0] - 1
    M, m = np.zeros((n, 3, 3)), np.zeros((n, 3))
    for q in range(n):
        Ast = As[q].T
        M[q] = _mat3(Ast, A[q])
        if translation:
            S = np.float64(np.asarray(scales, dtype=np.float64).reshape(-1)[q])
            assert np.isfinite(S) and S > 0
            m[q] = _matvec(Ast, c[q] - cs[q]) / S
    return M, m


def forward_map(z, R, t, fx, fy, cx, cy, M, m, mode=0, q5_mode=0):
    """Stage B with the virtual pose.  -> gx, gy (float64), D (rows, cols, 2) float32"""
    rows, cols = z.shape
    R = np.asarray(R, dtype=np.float64).reshape(rows, 9)
    t = np.asarray(t, dtype=np.float64).reshape(rows, 3)
    M = np.asarray(M, dtype=np.float64).reshape(9)
    m = np.asarray(m, dtype=np.float64).reshape(3)
    fyp = fx if q5_mode == 0 else fy
    ys = np.arange(rows) if mode == 0 else np.zeros(rows, dtype=np.int64)
    Rs, ts = R[ys][:, None, :], t[ys][:, None, :]
    R0, t0 = R[0], t[0]
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        nx = (x - cx) * 1.0 / fx
        ny = (y - cy) * 1.0 / fy
        pc = [z * nx, z * ny, z * 1.0]
        pw = []
        for i in range(3):
            rt0, rt1, rt2 = Rs[..., i], Rs[..., 3 + i], Rs[..., 6 + i]
            ti = ((-rt0) * ts[..., 0] + (-rt1) * ts[..., 1]) + (-rt2) * ts[..., 2]
            pw.append(((rt0 * pc[0] + rt1 * pc[1]) + rt2 * pc[2]) + ti * 1.0)
        pg = [((R0[3 * i] * pw[0] + R0[3 * i + 1] * pw[1]) + R0[3 * i + 2] * pw[2]) + t0[i] * 1.0 for i in range(3)]
        pv = [((M[3 * i] * pg[0] + M[3 * i + 1] * pg[1]) + M[3 * i + 2] * pg[2]) + m[i] for i in range(3)]
        gx = pv[0] / pv[2] * fx + cx
        gy = pv[1] / pv[2] * fyp + cy
        D = np.stack([(gx - x).astype(np.float32), (gy - y).astype(np.float32)], axis=-1)
    return gx, gy, np.ascontiguousarray(D)


def stabilize_frame(image, depth, R, t, K, M, m, mode=0, q5_mode=0, iterations=0):
    """the whole frame call.  depth (rows, cols); K = (fx, fy, cx, cy); iterations 0 = the dense default.
    -> dict(image, mask, filled (rows, cols) float64, disp (rows, cols, 2) float32, valid = int(mask.sum()))"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    it = iterations if iterations else dense.DEFAULT_ITERATIONS
    assert 1 <= it <= 16
    z = np.asarray(depth, dtype=np.float64)
    filled = dense.fill_depth(z)
    _, _, D = forward_map(filled, R, t, K[0], K[1], K[2], K[3], M, m, mode, q5_mode)
    if not dense.inverse_depth(z).any():  # no valid pixel: all-zero outputs
        return dict(image=np.zeros_like(image), mask=np.zeros(z.shape, dtype=np.uint8), filled=np.zeros_like(z), disp=D, valid=0)
    out, mask = dense.backward_warp(image, D, it)
    return dict(image=out, mask=mask, filled=filled, disp=D, valid=int(mask.sum()))
