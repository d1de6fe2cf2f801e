"""Executable definition of the stabiliser's search for the VISIBLE pre-image (include/rsdsfm_stabilize_search.h): where the occlusion test
(tests/stabilize_visible_spec_numpy.py) rejects a pixel because the neighbour's map folds there, the z-buffer knows which source pixel
landed on that cell; the fixed point is started again from that source pixel and, if it now ends on the near surface, the pixel is RECOVERED
instead of being left to the next candidate or to the inpainter.  The reference has no counterpart (main.cc:380-523 solves pairs one by one
and never relates them); this file is the definition and the kernels (csrc/stabilize_search_kernels.hip, compiled with -ffp-contract=off)
and host functions (csrc/stabilize_search_host.hip) reproduce it bit for bit.  tests/stabilize_visible_spec_numpy.py,
tests/stabilize_crop_spec_numpy.py, tests/stabilize_fill_spec_numpy.py, tests/stabilize_spec_numpy.py and tests/rectify_dense_spec_numpy.py
are imported and unchanged.

All arithmetic is float64 with one rounding per operation, sums taken in the order written.

forward_map_keys       visible.forward_map_depth (D and zv keep its bytes) with the uint32 z-buffer replaced by a plane of uint64 KEYS on the
                       virtual camera's grid, initialised to all ones: every source pixel (y, x) that splats there -- the same `inside`, the
                       same cell -- does kbuf[iy, ix] = min(kbuf[iy, ix], bits(zv) << 32 | (y cols + x)).  The minimum is the nearest depth
                       and, on equal depth, the smallest row-major source index: exact and independent of order.  kbuf >> 32 is the visible
                       spec's zbuf wherever a pixel landed and 0xFFFFFFFF where that holds +inf (asserted).
nearest_key            the minimum key over the in-frame part of the 3 x 3 block about the target's cell (visible.nearest_splat's block)
decide                 visible.visible's decision at a position against a given zn (the high word of the minimum key; all ones: no
                       evidence, visible)
fill_from_search       visible.fill_from_visible with a third outcome.  p, `valid` and the first test are the visible spec's.  A valid pixel
                       with mask 0 that passes is TAKEN with the visible call's bytes.  One that fails takes the search:
                         kn all ones: REJECTED.  Else (sy, sx) = divmod(low word of kn, cols), q = (sx, sy) as doubles, `iterations` steps
                         q <- t - bilinear(D, q) (the first fixed point's count and expressions), valid2 = the same four comparisons on q,
                         and the decision at q against the same zn.  valid2 and visible: RECOVERED -- saturate_u8(bilinear(image, q)), mask 1,
                         source source_id.  Otherwise REJECTED: image, mask and source keep what they had.
                       Pixels whose first fixed point is not valid are not offered; a candidate without one valid depth offers nothing and
                       counts nothing.  -> (taken, rejected, recovered): taken is the visible call's, rejected + recovered its rejected.

Not here: the own frame (id 1 keeps its call in the clips), targets whose first fixed point leaves the frame, the dense rectifier's own
folds, per-clip recovered counts, a tolerance derived from the depth's error.
"""
import numpy as np

import rectify_dense_spec_numpy as dense
import stabilize_crop_spec_numpy as crop
import stabilize_fill_spec_numpy as fill
import stabilize_spec_numpy as stab
import stabilize_visible_spec_numpy as visible

KEY_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
HIGH_EMPTY = np.uint32(0xFFFFFFFF)


def forward_map_keys(z, R, t, fx, fy, cx, cy, M, m, mode=0, q5_mode=0, _largest_index=False):
    """Stage B++ on the FILLED map z.  -> D, zv (visible.forward_map_depth's bytes), kbuf (rows, cols) uint64.  _largest_index: tests only --
    the other tie-break, the LARGEST source index among the nearest"""
    rows, cols = z.shape
    D, zv, zbuf = visible.forward_map_depth(z, R, t, fx, fy, cx, cy, M, m, mode, q5_mode)
    with np.errstate(all="ignore"):  # the same `inside` and the same cell as the z-buffer's splat
        gx, gy, _ = stab.forward_map(z, R, t, fx, fy, cx, cy, M, m, mode, q5_mode)
        inside = (zv > 0) & (gx >= -0.5) & (gx < cols - 0.5) & (gy >= -0.5) & (gy < rows - 0.5)
        ix = np.minimum(np.where(inside, gx + 0.5, 0.0).astype(np.int64), cols - 1)
        iy = np.minimum(np.where(inside, gy + 0.5, 0.0).astype(np.int64), rows - 1)
    index = np.arange(rows * cols, dtype=np.uint64).reshape(rows, cols)
    low = np.uint64(0xFFFFFFFF) - index if _largest_index else index  # (the minimum of the complement is the largest index)
    keys = (zv.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low
    kbuf = np.full((rows, cols), KEY_EMPTY, dtype=np.uint64)
    np.minimum.at(kbuf, (iy[inside], ix[inside]), keys[inside])
    if _largest_index:
        kbuf = np.where(kbuf == KEY_EMPTY, kbuf, (kbuf & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - (kbuf & np.uint64(0xFFFFFFFF))))
    high = (kbuf >> np.uint64(32)).astype(np.uint32)
    assert np.array_equal(high, np.where(zbuf == visible.ZBUF_EMPTY, HIGH_EMPTY, zbuf))
    return D, zv, kbuf


def nearest_key(kbuf, tx, ty):
    """-> kn (rows, cols) uint64: the minimum of kbuf over the in-frame 3 x 3 block about the target's cell"""
    rows, cols = kbuf.shape
    jc = np.minimum(np.maximum(tx + 0.5, 0.0), cols - 1.0).astype(np.int64)
    ic = np.minimum(np.maximum(ty + 0.5, 0.0), rows - 1.0).astype(np.int64)
    kn = np.full(tx.shape, KEY_EMPTY, dtype=np.uint64)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            i, j = ic + di, jc + dj
            ok = (i >= 0) & (i < rows) & (j >= 0) & (j < cols)
            kn = np.where(ok, np.minimum(kn, kbuf[np.clip(i, 0, rows - 1), np.clip(j, 0, cols - 1)]), kn)
    return kn


def decide(zv, high, px, py, tol_q16=0):
    """visible.visible's decision at (px, py) against zn = the float whose bits are `high` (all ones: no evidence).  -> bool"""
    k = visible.tolerance_factor(tol_q16)
    with np.errstate(all="ignore"):
        zs, some = visible.sampled_depth(zv, px, py)
        zn = np.where(high == HIGH_EMPTY, np.uint32(0), high).astype(np.uint32).view(np.float32)
        hidden = (high != HIGH_EMPTY) & (zs > zn.astype(np.float64) * k)
    return ~some & ~hidden


def stabilize_frame_search(image, depth, R, t, K, M, m, window, tol_q16=0, mode=0, q5_mode=0, iterations=0, _largest_index=False):
    """-> dict(image, mask: the window spec's, visible: the first test, image2: the sample at q, recovered (rows, cols) bool, disp, zv, kbuf)"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    it = iterations if iterations else dense.DEFAULT_ITERATIONS
    assert 1 <= it <= 16
    z = np.asarray(depth, dtype=np.float64)
    rows, cols = z.shape
    D, zv, kbuf = forward_map_keys(dense.fill_depth(z), R, t, K[0], K[1], K[2], K[3], M, m, mode, q5_mode, _largest_index)
    none = np.zeros(z.shape, dtype=bool)
    if not dense.inverse_depth(z).any():  # no valid pixel: the candidate offers nothing
        return dict(image=np.zeros_like(image), mask=np.zeros(z.shape, dtype=np.uint8), visible=none, image2=np.zeros_like(image), recovered=none, disp=D, zv=zv,
                    kbuf=kbuf)
    out, mask = crop.backward_warp_window(image, D, it, window)
    px, py = crop.inverse_positions_window(D, it, window)
    tx, ty = crop.window_targets(window, rows, cols)
    kn = nearest_key(kbuf, tx, ty)
    high = (kn >> np.uint64(32)).astype(np.uint32)
    first = decide(zv, high, px, py, tol_q16)
    low = (kn & np.uint64(0xFFFFFFFF)).astype(np.int64)
    low = np.where(kn == KEY_EMPTY, 0, low)
    sy, sx = np.divmod(low, cols)
    qx, qy = sx.astype(np.float64), sy.astype(np.float64)
    with np.errstate(all="ignore"):
        for _ in range(it):
            d = dense.bilinear(D, qx, qy)
            qx, qy = tx - d[..., 0], ty - d[..., 1]
        valid2 = (qx >= -0.5) & (qx < cols - 0.5) & (qy >= -0.5) & (qy < rows - 0.5)
        image2 = dense.saturate_u8(dense.bilinear(image, qx, qy)).astype(np.uint8)
    recovered = (mask == 1) & ~first & (kn != KEY_EMPTY) & valid2 & decide(zv, high, qx, qy, tol_q16)
    return dict(image=out, mask=mask, visible=first, image2=image2, recovered=recovered, disp=D, zv=zv, kbuf=kbuf)


def fill_from_search(out, mask, source, image_n, depth_n, R_n, t_n, K, M, m, source_id, window, tol_q16=0, mode=0, q5_mode=0, iterations=0, _largest_index=False):
    """one frame through the window, the test and the search: out, mask and source are changed IN PLACE where the mask is 0 and the pixel is
    taken or recovered.  -> (taken, rejected, recovered)"""
    assert 1 <= source_id <= 255
    cand = stabilize_frame_search(image_n, depth_n, R_n, t_n, K, M, m, window, tol_q16, mode, q5_mode, iterations, _largest_index)
    offered = (mask == 0) & (cand["mask"] == 1)
    take = offered & cand["visible"]
    again = offered & cand["recovered"]
    out[take] = cand["image"][take]
    out[again] = cand["image2"][again]
    mask[take | again] = 1
    source[take | again] = source_id
    return int(take.sum()), int(offered.sum()) - int(take.sum()) - int(again.sum()), int(again.sum())


def stabilize_cropped_frame_search(images, depths, Rs, ts, K, A, c, As, cs, scales, q, M_own, m_own, window, radius=fill.RADIUS_DEFAULT, tol_q16=0, mode=0,
                                   q5_mode=0, iterations=0):
    """visible.stabilize_cropped_frame_visible with every NEIGHBOUR (id >= 2) through the search; a recovered pixel counts under its offset.
    -> dict(image, mask, source, counts [none, own, -1, +1, ...] (2 + 2 radius), rejected, recovered: the neighbours' sums)"""
    npairs = len(depths)
    out = np.zeros_like(np.ascontiguousarray(images[q], dtype=np.uint8))
    rows, cols = out.shape[:2]
    mask, source = np.zeros((rows, cols), dtype=np.uint8), np.zeros((rows, cols), dtype=np.uint8)
    counts, rejected, recovered = [0] * (2 + 2 * radius), 0, 0
    if window[2] >= 1:
        counts[1] = crop.fill_from_window(out, mask, source, images[q], depths[q], Rs[q], ts[q], K, M_own, m_own, 1, window, mode, q5_mode, iterations)
        for n in (fill.neighbour_order(q, npairs, radius) if radius else []):
            sid = fill.source_id(n - q)
            M, m = fill.neighbour_pose(A, c, As, cs, scales, q, n)
            taken, rej, rec = fill_from_search(out, mask, source, images[n], depths[n], Rs[n], ts[n], K, M, m, sid, window, tol_q16, mode, q5_mode, iterations)
            counts[sid] = taken + rec
            rejected += rej
            recovered += rec
    counts[0] = mask.size - sum(counts[1:])
    return dict(image=out, mask=mask, source=source, counts=counts, rejected=rejected, recovered=recovered)
