"""Executable specification of the DeepFlow front end (csrc/flow_kernels.hip).

Two 8-bit images -> a dense flow field (rows x cols x 2, f64).  Every per-pixel quantity is float32 with one rounding per
operation, in the order written here; the HIP kernels evaluate the same expressions in the same order (-ffp-contract=off,
correctly rounded / and sqrt), so the device result is this function's result bit for bit.  Gaussian taps and resize
weights are computed in double and rounded to float once, as the host code does.
deep_flow(..., dtype=np.float64) is the same algorithm in double: the yardstick for what float32 costs (tests/test_flow_cpu.py).

The structure follows cv::optflow::createOptFlow_DeepFlow() of OpenCV 3.4 (recalled, not verified against its source):
one pre-smoothing, a bilinear pyramid with factor `downscale`, per level (coarse to fine) a variational refinement with
`fixed_point_iterations` outer and `sor_iterations` red-black SOR iterations, data term = brightness + gradient constancy
with Zimmer normalisation, smoothness = robust (Charbonnier) on forward differences.
"""
import math

import numpy as np

F = np.float32
ZETA2 = F(0.01)
EPS2 = F(1e-6)

DEFAULTS = dict(sigma=0.6, min_size=25, downscale=0.95, fixed_point_iterations=5, sor_iterations=25, alpha=1.0, delta=0.5, gamma=5.0,
                omega=1.6)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def flow_levels(rows, cols, downscale=0.95, min_size=25):
    """level 0 = full size; next = (int)(prev * downscale + 0.5) per axis; stop before a level with a side <= min_size or below 2 (a
    1x1 level has no neighbour and no derivative: its system is 0 * du = 0; 2 is also the smallest frame), or one that would not
    shrink at all"""
    levels = [(rows, cols)]
    while True:
        r, c = levels[-1]
        nr, nc = int(r * downscale + 0.5), int(c * downscale + 0.5)
        if nr <= min_size or nc <= min_size or nr < 2 or nc < 2 or (nr == r and nc == c):
            return levels
        levels.append((nr, nc))


def gray(img):
    """OpenCV's integer COLOR_BGR2GRAY for (rows, cols, 3) BGR; (rows, cols) or (rows, cols, 1) as is; -> float32"""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 3:
        b, g, r = (img[:, :, i].astype(np.int32) for i in range(3))
        return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(F)
    return img.reshape(img.shape[0], img.shape[1]).astype(F)


def gauss_taps(sigma):
    r = int(math.floor(3.0 * sigma))
    if r <= 0:
        return np.ones(1, dtype=F)
    g = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(-r, r + 1)]
    s = sum(g)
    return np.array([x / s for x in g], dtype=F)


def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.abs(i) % period
    return np.where(i >= n, period - i, i)


def smooth(f, taps):
    """separable Gaussian, border reflect-101: horizontal pass, then vertical; taps accumulated from the left / top"""
    rows, cols = f.shape
    r = len(taps) // 2
    xs, ys = np.arange(cols), np.arange(rows)
    h = taps[0] * f[:, reflect101(xs - r, cols)]
    for i in range(1, len(taps)):
        h = h + taps[i] * f[:, reflect101(xs - r + i, cols)]
    out = taps[0] * h[reflect101(ys - r, rows), :]
    for i in range(1, len(taps)):
        out = out + taps[i] * h[reflect101(ys - r + i, rows), :]
    return out


def resize_table(src, dst):
    """per destination index: (i0, i1, w0, w1); source coordinate (d + 0.5) * src / dst - 0.5 clamped to [0, src - 1], in double"""
    i0, i1, w0, w1 = [], [], [], []
    for d in range(dst):
        fx = (d + 0.5) * src / dst - 0.5
        fx = min(max(fx, 0.0), float(src - 1))
        a = int(math.floor(fx))
        t = fx - a
        i0.append(a)
        i1.append(min(a + 1, src - 1))
        w0.append(1.0 - t)
        w1.append(t)
    return np.array(i0), np.array(i1), np.array(w0, dtype=F), np.array(w1, dtype=F)


def resize(f, rows, cols):
    x0, x1, wx0, wx1 = resize_table(f.shape[1], cols)
    y0, y1, wy0, wy1 = resize_table(f.shape[0], rows)
    r0 = wx0[None, :] * f[y0][:, x0] + wx1[None, :] * f[y0][:, x1]
    r1 = wx0[None, :] * f[y1][:, x0] + wx1[None, :] * f[y1][:, x1]
    return wy0[:, None] * r0 + wy1[:, None] * r1


def warp(img, u, v):
    """bilinear sample of img at (x + u, y + v), coordinates clamped to [-1, side], replicate border"""
    rows, cols = img.shape
    X = np.fmin(np.fmax(np.arange(cols, dtype=F)[None, :] + u, F(-1)), F(cols))
    Y = np.fmin(np.fmax(np.arange(rows, dtype=F)[:, None] + v, F(-1)), F(rows))
    fx, fy = np.floor(X), np.floor(Y)
    ax, ay = X - fx, Y - fy
    bx, by = F(1) - ax, F(1) - ay
    xa = np.clip(fx.astype(np.int64), 0, cols - 1)
    xb = np.clip(fx.astype(np.int64) + 1, 0, cols - 1)
    ya = np.clip(fy.astype(np.int64), 0, rows - 1)
    yb = np.clip(fy.astype(np.int64) + 1, 0, rows - 1)
    r0 = bx * img[ya, xa] + ax * img[ya, xb]
    r1 = bx * img[yb, xa] + ax * img[yb, xb]
    return by * r0 + ay * r1


def dx(f):
    c = f.shape[1]
    xs = np.arange(c)
    return F(0.5) * (f[:, np.minimum(xs + 1, c - 1)] - f[:, np.maximum(xs - 1, 0)])


def dy(f):
    r = f.shape[0]
    ys = np.arange(r)
    return F(0.5) * (f[np.minimum(ys + 1, r - 1), :] - f[np.maximum(ys - 1, 0), :])


def derivatives(i1, i2w):
    avg = F(0.5) * (i1 + i2w)
    iz = i2w - i1
    ix, iy = dx(avg), dy(avg)
    return dict(Ix=ix, Iy=iy, Iz=iz, Ixx=dx(ix), Ixy=dy(ix), Iyy=dy(iy), Ixz=dx(iz), Iyz=dy(iz))


def _fwd(f, axis):
    """forward difference, 0 on the last row / column (replicate border)"""
    out = np.zeros_like(f)
    if axis == 1:
        out[:, :-1] = f[:, 1:] - f[:, :-1]
    else:
        out[:-1, :] = f[1:, :] - f[:-1, :]
    return out


def _nb(f):
    """(left, right, up, down) neighbours with replicate indices"""
    rows, cols = f.shape
    xs, ys = np.arange(cols), np.arange(rows)
    return (f[:, np.maximum(xs - 1, 0)], f[:, np.minimum(xs + 1, cols - 1)], f[np.maximum(ys - 1, 0), :], f[np.minimum(ys + 1, rows - 1), :])


def _nb0(f):
    """(left, right, up, down) neighbours, 0 outside the image"""
    p = np.pad(f, 1)
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def coefficients(d, u, v, du, dv, k):
    """the per-pixel 2x2 system of one fixed-point iteration: A12, R1 = 1 / (A11 + sum w), R2 = 1 / (A22 + sum w), B1, B2 (smoothness
    pull of (u, v) included) and the four neighbour weights (left, right, up, down)"""
    Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz = (d[n] for n in ("Ix", "Iy", "Iz", "Ixx", "Ixy", "Iyy", "Ixz", "Iyz"))
    n0 = (Ix * Ix + Iy * Iy) + ZETA2
    r0 = (Iz + Ix * du) + Iy * dv
    p0 = F(1) / np.sqrt((r0 * r0) / n0 + EPS2)
    k0 = (k["delta"] * p0) / n0
    nx = (Ixx * Ixx + Ixy * Ixy) + ZETA2
    ny = (Ixy * Ixy + Iyy * Iyy) + ZETA2
    rx = (Ixz + Ixx * du) + Ixy * dv
    ry = (Iyz + Ixy * du) + Iyy * dv
    pg = F(1) / np.sqrt(((rx * rx) / nx + (ry * ry) / ny) + EPS2)
    kx = (k["gamma"] * pg) / nx
    ky = (k["gamma"] * pg) / ny
    A11 = ((k0 * Ix) * Ix + (kx * Ixx) * Ixx) + (ky * Ixy) * Ixy
    A12 = ((k0 * Ix) * Iy + (kx * Ixx) * Ixy) + (ky * Ixy) * Iyy
    A22 = ((k0 * Iy) * Iy + (kx * Ixy) * Ixy) + (ky * Iyy) * Iyy
    b1 = -(((k0 * Ix) * Iz + (kx * Ixx) * Ixz) + (ky * Ixy) * Iyz)
    b2 = -(((k0 * Iy) * Iz + (kx * Ixy) * Ixz) + (ky * Iyy) * Iyz)
    U, V = u + du, v + dv
    ux, uy, vx, vy = _fwd(U, 1), _fwd(U, 0), _fwd(V, 1), _fwd(V, 0)
    s2 = ((ux * ux + uy * uy) + vx * vx) + vy * vy
    wgt = k["alpha"] * (F(1) / np.sqrt(s2 + EPS2))
    rows, cols = u.shape
    wR = wgt.copy()
    wR[:, cols - 1] = 0
    wD = wgt.copy()
    wD[rows - 1, :] = 0
    wL = np.zeros_like(wR)
    wL[:, 1:] = wR[:, :-1]
    wU = np.zeros_like(wD)
    wU[1:, :] = wD[:-1, :]
    W = ((wL + wR) + wU) + wD
    uL, uR, uU, uD = _nb(u)
    vL, vR, vU, vD = _nb(v)
    pu = ((wL * (uL - u) + wR * (uR - u)) + wU * (uU - u)) + wD * (uD - u)
    pv = ((wL * (vL - v) + wR * (vR - v)) + wU * (vU - v)) + wD * (vD - v)
    return dict(A12=A12, R1=F(1) / (A11 + W), R2=F(1) / (A22 + W), B1=b1 + pu, B2=b2 + pv, wL=wL, wR=wR, wU=wU, wD=wD)


def sor_half(c, du, dv, mask, k):
    """one red or black half-sweep: du first, then dv with the new du"""
    wL, wR, wU, wD = c["wL"], c["wR"], c["wU"], c["wD"]
    nL, nR, nU, nD = _nb0(du)
    s = ((wL * nL + wR * nR) + wU * nU) + wD * nD
    du_new = k["om1"] * du + k["om"] * (((c["B1"] + s) - c["A12"] * dv) * c["R1"])
    du = np.where(mask, du_new, du)
    nL, nR, nU, nD = _nb0(dv)
    s = ((wL * nL + wR * nR) + wU * nU) + wD * nD
    dv_new = k["om1"] * dv + k["om"] * (((c["B2"] + s) - c["A12"] * du) * c["R2"])
    return du, np.where(mask, dv_new, dv)


def constants(p):
    """the float32 constants the kernels receive (computed in double, rounded once)"""
    return dict(alpha=F(4.0 * p["alpha"]), delta=F(p["delta"] / 3.0), gamma=F(p["gamma"] / 3.0), om=F(p["omega"]), om1=F(1.0 - p["omega"]),
                scale=F(1.0 / p["downscale"]))


def deep_flow(img1, img2, dtype=F, **kw):
    """(rows, cols[, channels]) uint8 x 2 -> (rows, cols, 2) float64.  dtype=np.float64 runs the same algorithm with every per-pixel
    operation in double (the gray images and the zero fields start as float64 and every expression below follows its operands); the
    taps, the resize weights and the constants stay the float32 values the kernels receive, so the difference to the float32 run is
    the rounding of the per-pixel arithmetic alone"""
    p = params(**kw)
    k = constants(p)
    taps = gauss_taps(p["sigma"])
    a, b = smooth(gray(img1).astype(dtype), taps), smooth(gray(img2).astype(dtype), taps)
    rows, cols = a.shape
    levels = flow_levels(rows, cols, p["downscale"], p["min_size"])
    pyr = [(a, b)]
    for r, c in levels[1:]:
        pa, pb = pyr[-1]
        pyr.append((resize(pa, r, c), resize(pb, r, c)))
    u = v = None
    for li in range(len(levels) - 1, -1, -1):
        r, c = levels[li]
        i1, i2 = pyr[li]
        if u is None:
            u, v = np.zeros((r, c), dtype), np.zeros((r, c), dtype)
        else:
            u, v = resize(u, r, c) * k["scale"], resize(v, r, c) * k["scale"]
        d = derivatives(i1, warp(i2, u, v))
        du, dv = np.zeros((r, c), dtype), np.zeros((r, c), dtype)
        red = ((np.arange(r)[:, None] + np.arange(c)[None, :]) % 2) == 0
        for _ in range(p["fixed_point_iterations"]):
            co = coefficients(d, u, v, du, dv, k)
            for _ in range(p["sor_iterations"]):
                du, dv = sor_half(co, du, dv, red, k)
                du, dv = sor_half(co, du, dv, ~red, k)
        u, v = u + du, v + dv
    return np.stack([u, v], axis=-1).astype(np.float64)
