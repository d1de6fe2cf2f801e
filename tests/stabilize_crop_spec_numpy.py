"""Executable definition of the stabiliser's crop and zoom (include/rsdsfm_stabilize_crop.h): ONE window for the whole clip, found from the
masks the stabiliser already writes, and every frame rendered once, directly at the zoomed positions, through that window.  The reference has
no counterpart (main.cc:380-523 solves pairs one by one and never relates them); this file is the definition and the kernels
(csrc/stabilize_crop_kernels.hip, compiled with -ffp-contract=off) and host functions (csrc/stabilize_crop_host.hip) reproduce it bit for
bit.  tests/rectify_dense_spec_numpy.py, tests/stabilize_spec_numpy.py, tests/stabilize_fill_spec_numpy.py and tests/link_spec_numpy.py are
imported and unchanged.

The window is integer arithmetic only; everything else is float64 with one rounding per operation, sums taken in the order written.

crop_window            common = AND of the masks (0 is empty, anything else set).  A window of height h = 1 .. rows has width
                       w(h) = (h cols) // rows, the frame's aspect ratio floored; heights whose width is 0 do not exist.  Anchor (r, c) FITS h
                       iff r + h <= rows, c + w <= cols and the rectangle [r - margin, r + h + margin) x [c - margin, c + w + margin), clipped
                       to the frame, holds at most max_empty empty pixels of common (the frame's own edge is not a hole).  For one anchor
                       fitting is monotone in h (a smaller window's rectangle is nested in the larger one's): the largest fitting h is a binary
                       search on a summed-area table of the empties.  The answer: the largest h; ties by the smallest
                       |2 r + h - rows| + |2 c + w - cols| (nearest the centre, in doubled units), then the smallest r, then the smallest c.
                       Nothing fits: (0, 0, 0, 0).
window_targets         tx = (c0 + (ix + 0.5) (w / cols)) - 0.5, ty = (r0 + (iy + 0.5) (h / rows)) - 0.5, in that operation order: output
                       pixel g of the full-size frame, mapped into the window.  The full-frame window gives exactly the integers.
inverse_positions_window / backward_warp_window
                       the dense spec's stage C with the TARGET moved and D as it is: p = t, then p <- t - bilinear(D, p).  The contraction is
                       D's own, as without a zoom.  Validity, sampling and saturate_u8 unchanged; the output is rows x cols.
stabilize_frame_window the stabiliser's stabilize_frame with that stage C.
fill_from_window       the fill's fill_from with it; source_id 1 .. 255 (1: the own frame, rendered onto a zeroed mask).
stabilize_cropped_frame  frame q of a clip: zeroed planes, the own frame with id 1, then the neighbours in neighbour_order.

The horizontal and vertical scales differ because w is floored: less than one source pixel across the frame.  A fitted window does NOT
guarantee a full output mask: a target between two valid integer pixels can still leave the frame where the filled depth is rough.

Not here: windows that vary over time, path optimisers that trade smoothness against crop, a search that re-renders until the mask is
full, blending at seams, the clip's last frame.
"""
import numpy as np

import link_spec_numpy as link  # noqa: F401
import rectify_dense_spec_numpy as dense
import stabilize_fill_spec_numpy as fill
import stabilize_spec_numpy as stab

MARGIN_DEFAULT = 1  # pixels around the window that must be set as well: a choice, not a measurement
MARGIN_MAX = 64
PLANES_MAX = 4096


def window_width(h, rows, cols):
    return (h * cols) // rows


def common_mask(masks):
    """(planes, rows, cols) or a list of (rows, cols) -> bool (rows, cols): set in every plane"""
    m = np.asarray(masks)
    if m.ndim == 2:
        m = m[None]
    assert m.ndim == 3 and 1 <= m.shape[0] <= PLANES_MAX
    return (m != 0).all(axis=0)


def empties_table(common):
    """the summed-area table of the empties: (rows + 1, cols + 1) int64, row 0 and column 0 zero"""
    rows, cols = common.shape
    T = np.zeros((rows + 1, cols + 1), dtype=np.int64)
    T[1:, 1:] = (~common).astype(np.int64).cumsum(axis=1).cumsum(axis=0)
    return T


def fits(T, r, c, h, max_empty=0, margin=MARGIN_DEFAULT):
    """anchors r, c and heights h (integer arrays of one shape, h >= 1 with w(h) >= 1) -> bool"""
    rows, cols = T.shape[0] - 1, T.shape[1] - 1
    r, c, h = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64), np.asarray(h, dtype=np.int64)
    w = window_width(h, rows, cols)
    inside = (r + h <= rows) & (c + w <= cols)
    r0, r1 = np.clip(r - margin, 0, rows), np.clip(r + h + margin, 0, rows)
    c0, c1 = np.clip(c - margin, 0, cols), np.clip(c + w + margin, 0, cols)
    n = (T[r1, c1] - T[r0, c1]) - (T[r1, c0] - T[r0, c0])
    return inside & (n <= max_empty)


def largest_heights(T, max_empty=0, margin=MARGIN_DEFAULT):
    """-> (rows, cols) int64: every anchor's largest fitting height, 0 where none fits"""
    rows, cols = T.shape[0] - 1, T.shape[1] - 1
    r, c = np.mgrid[0:rows, 0:cols].astype(np.int64)
    hmin = (rows + cols - 1) // cols  # the smallest height with a width
    by_width = np.minimum(((cols - c + 1) * rows - 1) // cols, rows)  # the largest h with c + w(h) <= cols
    hi = np.minimum(rows - r, by_width)
    lo = np.full_like(hi, hmin - 1)  # "none"
    hi = np.maximum(hi, lo)
    for _ in range(15):  # heights <= 16384
        active = lo < hi
        mid = (lo + hi + 1) // 2  # > lo >= hmin - 1 where active
        ok = active & fits(T, r, c, np.maximum(mid, hmin), max_empty, margin)
        lo = np.where(ok, mid, lo)
        hi = np.where(active & ~ok, mid - 1, hi)
    assert np.array_equal(lo, hi)
    return np.where(lo >= hmin, lo, 0)


def window_key(r, c, h, rows, cols):
    """the 64-bit key whose maximum is the answer (Python integers or int64 arrays; sizes <= 16384: 60 bits)"""
    w = window_width(h, rows, cols)
    dist = abs(2 * r + h - rows) + abs(2 * c + w - cols)
    return (h << 45) | ((131071 - dist) << 28) | ((16383 - r) << 14) | (16383 - c)


def decode_key(key, rows, cols):
    key = int(key)
    if key == 0:
        return (0, 0, 0, 0)
    h = key >> 45
    return (16383 - ((key >> 14) & 16383), 16383 - (key & 16383), h, window_width(h, rows, cols))


def crop_window(masks, max_empty=0, margin=MARGIN_DEFAULT):
    """-> (r0, c0, h, w), Python integers"""
    common = common_mask(masks)
    rows, cols = common.shape
    assert 0 <= margin <= MARGIN_MAX and 0 <= max_empty <= rows * cols and 1 <= rows <= 16384 and 1 <= cols <= 16384
    H = largest_heights(empties_table(common), max_empty, margin)
    if not H.any():
        return (0, 0, 0, 0)
    r, c = np.mgrid[0:rows, 0:cols].astype(np.int64)
    keys = np.where(H > 0, window_key(r, c, H, rows, cols), 0)
    return decode_key(keys.max(), rows, cols)


def window_targets(window, rows, cols):
    """-> tx, ty (rows, cols) float64"""
    r0, c0, h, w = (int(v) for v in window)
    assert h >= 1 and w >= 1 and r0 >= 0 and c0 >= 0 and r0 + h <= rows and c0 + w <= cols
    iy, ix = np.mgrid[0:rows, 0:cols].astype(np.float64)
    sx, sy = np.float64(w) / np.float64(cols), np.float64(h) / np.float64(rows)
    return (np.float64(c0) + (ix + 0.5) * sx) - 0.5, (np.float64(r0) + (iy + 0.5) * sy) - 0.5


def inverse_positions_window(D, iterations, window):
    rows, cols = D.shape[:2]
    tx, ty = window_targets(window, rows, cols)
    px, py = tx, ty
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            d = dense.bilinear(D, px, py)
            px, py = tx - d[..., 0], ty - d[..., 1]
    return px, py


def backward_warp_window(image, D, iterations, window):
    """the dense spec's backward_warp at the window's targets.  -> (image, mask), rows x cols"""
    rows, cols = D.shape[:2]
    px, py = inverse_positions_window(D, iterations, window)
    with np.errstate(all="ignore"):
        valid = (px >= -0.5) & (px < cols - 0.5) & (py >= -0.5) & (py < rows - 0.5)
        val = dense.saturate_u8(dense.bilinear(image, px, py))
    out = np.where(valid[..., None] if image.ndim == 3 else valid, val, 0).astype(np.uint8)
    return out, valid.astype(np.uint8)


def stabilize_frame_window(image, depth, R, t, K, M, m, window, mode=0, q5_mode=0, iterations=0):
    """stab.stabilize_frame seen through the window.  -> dict(image, mask, filled, disp, valid)"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    it = iterations if iterations else dense.DEFAULT_ITERATIONS
    assert 1 <= it <= 16
    z = np.asarray(depth, dtype=np.float64)
    filled = dense.fill_depth(z)
    _, _, D = stab.forward_map(filled, R, t, K[0], K[1], K[2], K[3], M, m, mode, q5_mode)
    if not dense.inverse_depth(z).any():  # no valid pixel: all-zero outputs
        return dict(image=np.zeros_like(image), mask=np.zeros(z.shape, dtype=np.uint8), filled=np.zeros_like(z), disp=D, valid=0)
    out, mask = backward_warp_window(image, D, it, window)
    return dict(image=out, mask=mask, filled=filled, disp=D, valid=int(mask.sum()))


def fill_from_window(out, mask, source, image_n, depth_n, R_n, t_n, K, M, m, source_id, window, mode=0, q5_mode=0, iterations=0):
    """one frame through the window: out, mask and source are changed IN PLACE where the mask is 0 and the candidate is valid.  -> the number
    of pixels taken"""
    assert 1 <= source_id <= 255
    cand = stabilize_frame_window(image_n, depth_n, R_n, t_n, K, M, m, window, mode=mode, q5_mode=q5_mode, iterations=iterations)
    take = (mask == 0) & (cand["mask"] == 1)
    out[take] = cand["image"][take]
    mask[take] = 1
    source[take] = source_id
    return int(take.sum())


def stabilize_cropped_frame(images, depths, Rs, ts, K, A, c, As, cs, scales, q, M_own, m_own, window, radius=fill.RADIUS_DEFAULT, mode=0, q5_mode=0,
                            iterations=0):
    """frame q of a clip through the window: zeroed planes, the own frame (id 1), then fill.neighbour_order's candidates (radius 0: none).
    -> dict(image, mask, source, counts [none, own, -1, +1, ...] (2 + 2 radius))"""
    npairs = len(depths)
    out = np.zeros_like(np.ascontiguousarray(images[q], dtype=np.uint8))
    rows, cols = out.shape[:2]
    mask, source = np.zeros((rows, cols), dtype=np.uint8), np.zeros((rows, cols), dtype=np.uint8)
    counts = [0] * (2 + 2 * radius)
    if window[2] >= 1:
        counts[1] = fill_from_window(out, mask, source, images[q], depths[q], Rs[q], ts[q], K, M_own, m_own, 1, window, mode, q5_mode, iterations)
        for n in (fill.neighbour_order(q, npairs, radius) if radius else []):
            sid = fill.source_id(n - q)
            M, m = fill.neighbour_pose(A, c, As, cs, scales, q, n)
            counts[sid] = fill_from_window(out, mask, source, images[n], depths[n], Rs[n], ts[n], K, M, m, sid, window, mode, q5_mode, iterations)
    counts[0] = mask.size - sum(counts[1:])
    return dict(image=out, mask=mask, source=source, counts=counts)
