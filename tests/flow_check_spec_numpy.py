"""The forward-backward flow check (include/rsdsfm_flow_check.h; Sundaram, Brox, Keutzer, ECCV 2010), defined in float64 numpy: the
kernel of csrc/flow_check_kernels.hip reproduces it bit for bit.  Every operation is rounded once and none is fused (the library is
built with -ffp-contract=off).

fwd is the field frame 1 -> frame 2, bwd the field frame 2 -> frame 1, both rows x cols x 2 doubles, (u, v) per pixel, row-major.  For
pixel (row i, column j) with (u, v) = fwd[i, j]:
    1  px = j + u, py = i + v; the pixel is INSIDE iff 0 <= px <= cols - 1 and 0 <= py <= rows - 1 (false for NaN)
    2  x0 = min(floor(px), cols - 2), ax = px - x0; y0, ay likewise (a landing point on the last column / row has ax = 1 / ay = 1)
    3  (bu, bv) = the bilinear sample of bwd, per component:  top = b00 + ax * (b01 - b00), bot = b10 + ax * (b11 - b10),
       val = top + ay * (bot - top)
    4  r = (u + bu) * (u + bu) + (v + bv) * (v + bv)
    5  bound = a1 * ((u * u + v * v) + (bu * bu + bv * bv)) + a2
    6  mask = 1 iff inside and r <= bound (false for NaN: a non-finite tap rejects the pixel)
    7  resid = r where inside and r is finite, else +inf
    8  masked[i, j] = (u, v) where mask = 1, else (0.0, 0.0)
    9  count = the number of ones
"""
import numpy as np

A1_DEFAULT, A2_DEFAULT = 0.01, 0.5


def flow_check(fwd, bwd, a1=A1_DEFAULT, a2=A2_DEFAULT):
    """-> dict(mask (rows, cols) uint8, masked (rows, cols, 2) float64, resid (rows, cols) float64, count int)"""
    fwd, bwd = np.asarray(fwd, dtype=np.float64), np.asarray(bwd, dtype=np.float64)
    rows, cols = fwd.shape[:2]
    assert fwd.shape == bwd.shape == (rows, cols, 2) and rows >= 2 and cols >= 2
    a1, a2 = np.float64(a1), np.float64(a2)
    u, v = fwd[..., 0], fwd[..., 1]
    ii, jj = np.mgrid[0:rows, 0:cols].astype(np.float64)
    with np.errstate(all="ignore"):
        px, py = jj + u, ii + v
        inside = (px >= 0.0) & (px <= cols - 1.0) & (py >= 0.0) & (py <= rows - 1.0)
        sx, sy = np.where(inside, px, 0.0), np.where(inside, py, 0.0)  # (pixels that are not inside take no tap: any position will do)
        x0 = np.minimum(np.floor(sx), cols - 2.0)
        y0 = np.minimum(np.floor(sy), rows - 2.0)
        ax, ay = sx - x0, sy - y0
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        b = []
        for comp in range(2):
            f = bwd[..., comp]
            b00, b01, b10, b11 = f[y0, x0], f[y0, x0 + 1], f[y0 + 1, x0], f[y0 + 1, x0 + 1]
            top = b00 + ax * (b01 - b00)
            bot = b10 + ax * (b11 - b10)
            b.append(top + ay * (bot - top))
        bu, bv = b
        r = (u + bu) * (u + bu) + (v + bv) * (v + bv)
        bound = a1 * ((u * u + v * v) + (bu * bu + bv * bv)) + a2
        mask = inside & (r <= bound)
        resid = np.where(inside & np.isfinite(r), r, np.inf)
    masked = np.where(mask[..., None], fwd, 0.0)
    return dict(mask=mask.astype(np.uint8), masked=np.ascontiguousarray(masked), resid=resid, count=int(mask.sum()))
