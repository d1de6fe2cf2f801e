"""Executable definition of the dense global-shutter rectifier (include/rsdsfm_rectify_dense.h): inverse-depth fill, forward map and
backward warp, in numpy.  It plays the role tests/flow_spec_numpy.py plays for DeepFlow: every intermediate has a fixed type and every
operation one rounding, and the HIP kernels (csrc/rectify_dense_kernels.hip, compiled with -ffp-contract=off) reproduce it bit for bit.

Types: all arithmetic in float64; the displacement plane D is stored as float32 pairs (the one narrowing), frame and mask are bytes.
Linear interpolation is always  lerp(a, b, t) = a + t * (b - a)  (x first, then y): it returns a exactly when a == b, and for
0 <= t <= 3/4 it stays inside [a, b], so a fill never leaves the range of the valid values.

Stage A  fill_depth       rho = 1 / z where z is finite, z > 0 and 1 / z > 0, else 0 (0 = invalid: no weight plane).  Pull: a cell of
                          level l + 1 (ceil(h / 2) x ceil(w / 2)) is the mean of its n non-zero children (absent ones are 0), taken about
                          the first of them, a:  a + (((c00 - a) + (c01 - a)) + (c10 - a)) + (c11 - a)) / n  without the terms of the
                          zero children -- equal children give their value exactly, which a plain sum / 3 does not --, or 0 if n = 0;
                          down to 1 x 1.  Push, coarse to fine: a cell that is 0 takes the
                          bilinear value of the complete coarser level at ((x + 1/2) / 2 - 1/2, (y + 1/2) / 2 - 1/2), clamped to the
                          level, neighbour min(i0 + 1, n - 1).  z_filled = z at a valid pixel (not 1 / (1 / z)), 1 / rho at a filled
                          one, 0 when the map has no valid pixel (the 1 x 1 level is 0).
Stage B  forward_map      back_project_claim_body's chain (rectify_kernels.hip; oracle/rsdsfm_oracle.c rso_back_project) for every
                          pixel, the marker colour included, on z_filled: (gx, gy) in float64, D = (float32(gx - x), float32(gy - y)).
Stage C  backward_warp    p_0 = g, p_{n+1} = g - D(p_n) with D bilinear (replicate border), exactly `iterations` steps; the pixel is
                          valid iff -1/2 <= p_x < cols - 1/2 and -1/2 <= p_y < rows - 1/2 (false for NaN / inf); a valid pixel is the
                          bilinear sample of the frame at p clamped to the frame, rounded to nearest even and clamped to 0..255.
clamp(p, n) is  (p > 0 ? p : 0) < n - 1 ? . : n - 1  -- NaN and -inf go to 0, +inf to n - 1.
"""
import numpy as np

DEFAULT_ITERATIONS = 3


def _clamp(p, n):
    c = np.where(p > 0.0, p, 0.0)
    return np.where(c < n - 1.0, c, n - 1.0)


def _lerp(a, b, t):
    return a + t * (b - a)


def bilinear(plane, px, py):
    """plane (h, w) or (h, w, C) of any real type, converted to float64, at float64 positions (px, py): replicate border"""
    h, w = plane.shape[:2]
    cx, cy = _clamp(px, w), _clamp(py, h)
    x0, y0 = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = cx - x0, cy - y0
    if plane.ndim == 3:
        ax, ay = ax[..., None], ay[..., None]
    f = lambda yy, xx: plane[yy, xx].astype(np.float64)
    return _lerp(_lerp(f(y0, x0), f(y0, x1), ax), _lerp(f(y1, x0), f(y1, x1), ax), ay)


def inverse_depth(depth):
    z = np.asarray(depth, dtype=np.float64)
    with np.errstate(all="ignore"):
        rho = 1.0 / z
        ok = np.isfinite(z) & (z > 0.0) & (rho > 0.0)
    return np.where(ok, rho, 0.0)


def pull(level):
    """one pull step: (h, w) -> (ceil(h / 2), ceil(w / 2))"""
    h, w = level.shape
    p = np.zeros((2 * ((h + 1) // 2), 2 * ((w + 1) // 2)))
    p[:h, :w] = level
    c00, c01, c10, c11 = p[0::2, 0::2], p[0::2, 1::2], p[1::2, 0::2], p[1::2, 1::2]
    a = np.where(c00 != 0, c00, np.where(c01 != 0, c01, np.where(c10 != 0, c10, c11)))  # the first non-zero child
    d = lambda c: np.where(c != 0, c - a, 0.0)
    s = ((d(c00) + d(c01)) + d(c10)) + d(c11)
    n = (c00 != 0).astype(np.float64) + (c01 != 0) + (c10 != 0) + (c11 != 0)
    with np.errstate(all="ignore"):
        return np.where(n > 0, a + s / n, 0.0)


def push(level, coarser):
    """one push step: the cells of `level` that are 0 take the bilinear value of the complete `coarser` level"""
    h, w = level.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.where(level != 0, level, bilinear(coarser, (xx + 0.5) * 0.5 - 0.5, (yy + 0.5) * 0.5 - 0.5))


def fill_inverse_depth(rho0):
    """push-pull on the inverse depth: the complete level 0 and the 1 x 1 level's value (0: no valid pixel)"""
    levels = [rho0]
    while levels[-1].shape != (1, 1):
        levels.append(pull(levels[-1]))
    done = levels[-1]
    for lv in levels[-2::-1]:
        done = push(lv, done)
    return done, float(levels[-1][0, 0])


def fill_depth(depth):
    """Stage A.  depth (rows, cols) -> z_filled (rows, cols)"""
    z = np.asarray(depth, dtype=np.float64)
    rho0 = inverse_depth(z)
    rho, _ = fill_inverse_depth(rho0)
    with np.errstate(all="ignore"):
        return np.where(rho0 != 0, z, np.where(rho > 0.0, 1.0 / rho, 0.0))


def forward_map(z, R, t, fx, fy, cx, cy, mode=0, q5_mode=0, want_world=False):
    """Stage B.  z (rows, cols), R (rows, 9) / (rows, 3, 3), t (rows, 3) -> gx, gy (float64) and D (rows, cols, 2) float32; want_world: also
    the chain's world points (rows, cols, 3) float64, what the splat exports as float32 (d_coords3d)"""
    rows, cols = z.shape
    R = np.asarray(R, dtype=np.float64).reshape(rows, 9)
    t = np.asarray(t, dtype=np.float64).reshape(rows, 3)
    fyp = fx if q5_mode == 0 else fy
    ys = np.arange(rows) if mode == 0 else np.zeros(rows, dtype=np.int64)
    Rs, ts = R[ys][:, None, :], t[ys][:, None, :]  # per scanline, broadcast along x
    R0, t0 = R[0], t[0]
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        nx = (x - cx) * 1.0 / fx
        ny = (y - cy) * 1.0 / fy
        pc = [z * nx, z * ny, z * 1.0]
        pw = []
        for i in range(3):
            rt0, rt1, rt2 = Rs[..., i], Rs[..., 3 + i], Rs[..., 6 + i]  # row i of R^T
            ti = ((-rt0) * ts[..., 0] + (-rt1) * ts[..., 1]) + (-rt2) * ts[..., 2]
            pw.append(((rt0 * pc[0] + rt1 * pc[1]) + rt2 * pc[2]) + ti * 1.0)
        pg = [((R0[3 * i] * pw[0] + R0[3 * i + 1] * pw[1]) + R0[3 * i + 2] * pw[2]) + t0[i] * 1.0 for i in range(3)]
        gx = pg[0] / pg[2] * fx + cx
        gy = pg[1] / pg[2] * fyp + cy
        D = np.stack([(gx - x).astype(np.float32), (gy - y).astype(np.float32)], axis=-1)
    if want_world:
        return gx, gy, np.ascontiguousarray(D), np.stack(pw, axis=-1)
    return gx, gy, np.ascontiguousarray(D)


def inverse_positions(D, iterations=DEFAULT_ITERATIONS):
    """the fixed point of stage C: p (rows, cols, 2) float64 after exactly `iterations` steps"""
    rows, cols = D.shape[:2]
    gy, gx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    px, py = gx, gy
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            d = bilinear(D, px, py)
            px, py = gx - d[..., 0], gy - d[..., 1]
    return px, py


def saturate_u8(v):
    """cvRound (nearest even) + clamp, as the splat's saturate_u8"""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def backward_warp(image, D, iterations=DEFAULT_ITERATIONS):
    """Stage C.  image (rows, cols) or (rows, cols, 3) uint8 -> (dense image, mask)"""
    rows, cols = D.shape[:2]
    px, py = inverse_positions(D, iterations)
    with np.errstate(all="ignore"):
        valid = (px >= -0.5) & (px < cols - 0.5) & (py >= -0.5) & (py < rows - 0.5)
        val = saturate_u8(bilinear(image, px, py))  # (the clamped position is finite whatever p is)
    out = np.where(valid[..., None] if image.ndim == 3 else valid, val, 0).astype(np.uint8)
    return out, valid.astype(np.uint8)


def rectify_dense(image, depth, R, t, fx, fy, cx, cy, mode=0, q5_mode=0, iterations=0):
    """the whole call.  depth: (rows, cols) array (the C ABI takes it column-major); iterations 0 = DEFAULT_ITERATIONS.
    Returns dict(image, mask, filled (rows, cols) float64, disp (rows, cols, 2) float32)"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    it = iterations if iterations else DEFAULT_ITERATIONS
    assert 1 <= it <= 16
    z = np.asarray(depth, dtype=np.float64)
    filled = fill_depth(z)
    _, _, D = forward_map(filled, R, t, fx, fy, cx, cy, mode, q5_mode)
    if not inverse_depth(z).any():  # no valid pixel: all-zero outputs
        return dict(image=np.zeros_like(image), mask=np.zeros(z.shape, dtype=np.uint8), filled=np.zeros_like(z), disp=D)
    out, mask = backward_warp(image, D, it)
    return dict(image=out, mask=mask, filled=filled, disp=D)
