"""Executable definition of the stabiliser's occlusion test (include/rsdsfm_stabilize_visible.h): a neighbour frame rendered into a virtual
camera offers a pixel only when the source pixel stage C found is the one NEAREST THE CAMERA among those that land there.  The reference has
no counterpart (main.cc:380-523 solves pairs one by one and never relates them); this file is the definition and the kernels
(csrc/stabilize_visible_kernels.hip, compiled with -ffp-contract=off) and host functions (csrc/stabilize_visible_host.hip) reproduce it bit
for bit.  tests/stabilize_crop_spec_numpy.py, tests/stabilize_fill_spec_numpy.py, tests/stabilize_spec_numpy.py and
tests/rectify_dense_spec_numpy.py are imported and unchanged.

Stage C inverts the displacement plane D by p <- t - D(p) from p = t.  Where the neighbour's map folds -- a near surface has moved in front
of a far one -- a target has two pre-images and the iteration finds the one nearer in the image plane, not the one nearer the camera: the
far surface is painted over the near one.  The test rejects such a pixel; the next candidate, or the inpainter, takes it.

All arithmetic is float64 with one rounding per operation, sums taken in the order written.

forward_map_depth      stab.forward_map's chain (D keeps its bytes) and two more planes:
                         zv    float32, the source grid: (float)pv[2] where pv[2] > 0, pv[2] is finite and the float is finite, else 0
                         zbuf  uint32, the VIRTUAL CAMERA's own pixel grid (whatever window is used later), initialised to 0x7f800000
                               (+inf): every source pixel with zv > 0, -0.5 <= gx < cols - 0.5 and -0.5 <= gy < rows - 0.5 (false for
                               NaN) does zbuf[iy, ix] = min(zbuf[iy, ix], bits(zv)), ix = min((int)(gx + 0.5), cols - 1), iy likewise;
                               gx, gy are the doubles of the projection, not the rounded floats of D.  Positive floats order as their
                               bit patterns: the minimum is exact and independent of order.
visible                the decision for a target t = (tx, ty) whose fixed point is p (valid as today):
                         zs    the four taps of zv at the taps of the image sample; any of them 0: REJECTED; else
                               lerp(lerp(z00, z01, ax), lerp(z10, z11, ax), ay)
                         zn    the minimum of zbuf over the in-frame part of the 3 x 3 block about (ic, jc),
                               jc = (int)min(max(tx + 0.5, 0), cols - 1), ic likewise from ty
                         zn == +inf: nothing was splatted there, no evidence: visible.  Otherwise rejected iff zs > (double)zn k,
                         k = 1.0 + tol_q16 / 65536.0, computed once.
fill_from_visible      crop.fill_from_window with the decision: a rejected pixel is not taken, image, mask and source keep what they had.
                       Pixels whose mask is set are neither tested nor counted; a candidate without one valid depth offers nothing and
                       counts nothing.  -> (taken, rejected)

The 3 x 3 block covers the splat's cracks and the float rounding of D; it erodes a depth edge by one pixel.  TOL_Q16_DEFAULT = 3277
(about 0.05) is a choice, not a measurement.

Not here: searching for the VISIBLE pre-image instead of rejecting, the own frame (id 1 keeps its call in the clips), the dense rectifier's
own folds, per-clip rejected counts.
"""
import numpy as np

import rectify_dense_spec_numpy as dense
import stabilize_crop_spec_numpy as crop
import stabilize_fill_spec_numpy as fill
import stabilize_spec_numpy as stab

TOL_Q16_DEFAULT = 3277  # about 0.05 of the depth: a choice, not a measurement
TOL_Q16_MAX = 65536
ZBUF_EMPTY = np.uint32(0x7F800000)  # +inf


def tolerance_factor(tol_q16=0):
    """k = 1.0 + tol_q16 / 65536.0 (0: the default)"""
    q = int(tol_q16) if tol_q16 else TOL_Q16_DEFAULT
    assert 1 <= q <= TOL_Q16_MAX
    return np.float64(1.0) + np.float64(q) / np.float64(65536.0)


def forward_map_depth(z, R, t, fx, fy, cx, cy, M, m, mode=0, q5_mode=0):
    """Stage B+ on the FILLED map z.  -> D (rows, cols, 2) float32 (stab.forward_map's bytes), zv (rows, cols) float32, zbuf (rows, cols) uint32"""
    rows, cols = z.shape
    R = np.asarray(R, dtype=np.float64).reshape(rows, 9)
    t = np.asarray(t, dtype=np.float64).reshape(rows, 3)
    M = np.asarray(M, dtype=np.float64).reshape(9)
    m = np.asarray(m, dtype=np.float64).reshape(3)
    ys = np.arange(rows) if mode == 0 else np.zeros(rows, dtype=np.int64)
    Rs, ts = R[ys][:, None, :], t[ys][:, None, :]
    R0, t0 = R[0], t[0]
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):  # stab.forward_map's chain up to pv, operation for operation
        nx = (x - cx) * 1.0 / fx
        ny = (y - cy) * 1.0 / fy
        pc = [z * nx, z * ny, z * 1.0]
        pw = []
        for i in range(3):
            rt0, rt1, rt2 = Rs[..., i], Rs[..., 3 + i], Rs[..., 6 + i]
            ti = ((-rt0) * ts[..., 0] + (-rt1) * ts[..., 1]) + (-rt2) * ts[..., 2]
            pw.append(((rt0 * pc[0] + rt1 * pc[1]) + rt2 * pc[2]) + ti * 1.0)
        pg = [((R0[3 * i] * pw[0] + R0[3 * i + 1] * pw[1]) + R0[3 * i + 2] * pw[2]) + t0[i] * 1.0 for i in range(3)]
        pv2 = np.broadcast_to(((M[6] * pg[0] + M[7] * pg[1]) + M[8] * pg[2]) + m[2], (rows, cols))
        gx, gy, D = stab.forward_map(z, R, t, fx, fy, cx, cy, M, m, mode, q5_mode)
        zf = pv2.astype(np.float32)
        zv = np.where((pv2 > 0.0) & np.isfinite(pv2) & np.isfinite(zf), zf, np.float32(0.0)).astype(np.float32)
        inside = (zv > 0) & (gx >= -0.5) & (gx < cols - 0.5) & (gy >= -0.5) & (gy < rows - 0.5)
        ix = np.minimum(np.where(inside, gx + 0.5, 0.0).astype(np.int64), cols - 1)
        iy = np.minimum(np.where(inside, gy + 0.5, 0.0).astype(np.int64), rows - 1)
    zbuf = np.full((rows, cols), ZBUF_EMPTY, dtype=np.uint32)
    np.minimum.at(zbuf, (iy[inside], ix[inside]), zv.view(np.uint32)[inside])
    return D, zv, zbuf


def sampled_depth(zv, px, py):
    """-> zs (float64; meaningless where some is False), some: one of the four taps is 0"""
    rows, cols = zv.shape
    cx, cy = dense._clamp(px, cols), dense._clamp(py, rows)
    x0, y0 = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, cols - 1), np.minimum(y0 + 1, rows - 1)
    ax, ay = cx - x0, cy - y0
    z00, z01, z10, z11 = (zv[a, b].astype(np.float64) for a, b in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    some = (z00 == 0) | (z01 == 0) | (z10 == 0) | (z11 == 0)
    return dense._lerp(dense._lerp(z00, z01, ax), dense._lerp(z10, z11, ax), ay), some


def nearest_splat(zbuf, tx, ty):
    """-> zn (rows, cols) float32: the minimum of zbuf over the in-frame 3 x 3 block about the target's cell"""
    rows, cols = zbuf.shape
    jc = np.minimum(np.maximum(tx + 0.5, 0.0), cols - 1.0).astype(np.int64)
    ic = np.minimum(np.maximum(ty + 0.5, 0.0), rows - 1.0).astype(np.int64)
    zn = np.full(tx.shape, ZBUF_EMPTY, dtype=np.uint32)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            i, j = ic + di, jc + dj
            ok = (i >= 0) & (i < rows) & (j >= 0) & (j < cols)
            zn = np.where(ok, np.minimum(zn, zbuf[np.clip(i, 0, rows - 1), np.clip(j, 0, cols - 1)]), zn)
    return zn.astype(np.uint32).view(np.float32)


def visible(zv, zbuf, px, py, tx, ty, tol_q16=0):
    """-> bool (rows, cols): the pixel passes the test (to be ANDed with stage C's validity)"""
    k = tolerance_factor(tol_q16)
    with np.errstate(all="ignore"):
        zs, some = sampled_depth(zv, px, py)
        zn = nearest_splat(zbuf, tx, ty)
        hidden = ~np.isinf(zn) & (zs > zn.astype(np.float64) * k)
    return ~some & ~hidden


def stabilize_frame_visible(image, depth, R, t, K, M, m, window, tol_q16=0, mode=0, q5_mode=0, iterations=0):
    """crop.stabilize_frame_window plus the decision.  -> dict(image, mask: the window spec's, visible (rows, cols) bool, disp, zv, zbuf)"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    it = iterations if iterations else dense.DEFAULT_ITERATIONS
    assert 1 <= it <= 16
    z = np.asarray(depth, dtype=np.float64)
    rows, cols = z.shape
    D, zv, zbuf = forward_map_depth(dense.fill_depth(z), R, t, K[0], K[1], K[2], K[3], M, m, mode, q5_mode)
    if not dense.inverse_depth(z).any():  # no valid pixel: the candidate offers nothing
        return dict(image=np.zeros_like(image), mask=np.zeros(z.shape, dtype=np.uint8), visible=np.zeros(z.shape, dtype=bool), disp=D, zv=zv, zbuf=zbuf)
    out, mask = crop.backward_warp_window(image, D, it, window)
    px, py = crop.inverse_positions_window(D, it, window)
    tx, ty = crop.window_targets(window, rows, cols)
    return dict(image=out, mask=mask, visible=visible(zv, zbuf, px, py, tx, ty, tol_q16), disp=D, zv=zv, zbuf=zbuf)


def fill_from_visible(out, mask, source, image_n, depth_n, R_n, t_n, K, M, m, source_id, window, tol_q16=0, mode=0, q5_mode=0, iterations=0):
    """one frame through the window and the test: out, mask and source are changed IN PLACE where the mask is 0, the candidate is valid and
    visible.  -> (taken, rejected)"""
    assert 1 <= source_id <= 255
    cand = stabilize_frame_visible(image_n, depth_n, R_n, t_n, K, M, m, window, tol_q16, mode, q5_mode, iterations)
    offered = (mask == 0) & (cand["mask"] == 1)
    take = offered & cand["visible"]
    out[take] = cand["image"][take]
    mask[take] = 1
    source[take] = source_id
    return int(take.sum()), int(offered.sum()) - int(take.sum())


def stabilize_cropped_frame_visible(images, depths, Rs, ts, K, A, c, As, cs, scales, q, M_own, m_own, window, radius=fill.RADIUS_DEFAULT, tol_q16=0, mode=0,
                                    q5_mode=0, iterations=0):
    """crop.stabilize_cropped_frame with every NEIGHBOUR (id >= 2) through the test; the own frame keeps crop.fill_from_window.
    -> dict(image, mask, source, counts [none, own, -1, +1, ...] (2 + 2 radius), rejected: the neighbours' sum)"""
    npairs = len(depths)
    out = np.zeros_like(np.ascontiguousarray(images[q], dtype=np.uint8))
    rows, cols = out.shape[:2]
    mask, source = np.zeros((rows, cols), dtype=np.uint8), np.zeros((rows, cols), dtype=np.uint8)
    counts, rejected = [0] * (2 + 2 * radius), 0
    if window[2] >= 1:
        counts[1] = crop.fill_from_window(out, mask, source, images[q], depths[q], Rs[q], ts[q], K, M_own, m_own, 1, window, mode, q5_mode, iterations)
        for n in (fill.neighbour_order(q, npairs, radius) if radius else []):
            sid = fill.source_id(n - q)
            M, m = fill.neighbour_pose(A, c, As, cs, scales, q, n)
            counts[sid], rej = fill_from_visible(out, mask, source, images[n], depths[n], Rs[n], ts[n], K, M, m, sid, window, tol_q16, mode, q5_mode, iterations)
            rejected += rej
    counts[0] = mask.size - sum(counts[1:])
    return dict(image=out, mask=mask, source=source, counts=counts, rejected=rejected)
