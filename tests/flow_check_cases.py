"""Inputs of the flow check's tests (tests/test_flow_check_cpu.py, tests/test_gpu_flow_check.py) and of its golden fixture
(tests/golden/make_golden_flow_check.py): a forward and a backward field per shape with everything the check distinguishes."""
import numpy as np

SHAPES = [(2, 2), (5, 3), (16, 64), (33, 68), (33, 70), (150, 200)]  # (33, 70): 2310 pixels, a byte tail of 2; (150, 200): 118 workgroups


def bilinear(f, x, y):
    """f (rows, cols, 2) at real positions clamped into the frame (the spec's taps and order)"""
    rows, cols = f.shape[:2]
    x, y = np.clip(x, 0.0, cols - 1.0), np.clip(y, 0.0, rows - 1.0)
    x0, y0 = np.minimum(np.floor(x), cols - 2.0), np.minimum(np.floor(y), rows - 2.0)
    ax, ay = (x - x0)[..., None], (y - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    top = f[y0, x0] + ax * (f[y0, x0 + 1] - f[y0, x0])
    bot = f[y0 + 1, x0] + ax * (f[y0 + 1, x0 + 1] - f[y0 + 1, x0])
    return top + ay * (bot - top)


def smooth_field(rows, cols, rng, amp):
    """a few sinusoids per component, |component| <= amp"""
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    f = np.zeros((rows, cols, 2))
    for c in range(2):
        for _ in range(3):
            kx, ky = rng.uniform(-0.15, 0.15, 2)
            f[..., c] += np.sin(kx * xx + ky * yy + rng.uniform(0, 2 * np.pi))
    return f * (amp / 3.0)


def fields(rows, cols, specials=True):
    """(fwd, bwd, notes): bwd a smooth random field of up to 3 px per component (less on small frames); fwd its inverse by 30 fixed-point
    steps (f <- -bwd(p + f)) plus a smooth error of up to 0.45 px per component, so that most pixels are consistent; then a block of inconsistent vectors, vectors that leave the frame on
    all four sides and, with specials on frames of at least 5 x 3, the special values.  notes maps a name to the (row, column) it was
    put at."""
    rng = np.random.default_rng(1000 * rows + cols)
    amp = min(3.0, 0.2 * min(rows, cols))
    bwd = smooth_field(rows, cols, rng, amp)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    fwd = np.zeros_like(bwd)
    for _ in range(30):
        fwd = -bilinear(bwd, xx + fwd[..., 0], yy + fwd[..., 1])
    fwd += smooth_field(rows, cols, rng, 0.45)  # residuals from 0 to about 0.6 squared pixels: on both sides of the bound
    notes = {}
    if rows >= 16:  # a block of inconsistent vectors
        y0, x0, h, w = rows // 4, cols // 3, max(2, rows // 5), max(2, cols // 6)
        fwd[y0:y0 + h, x0:x0 + w] += np.array([2.5, -1.5])
        notes["block"] = (y0, x0, h, w)
    if rows >= 5 and cols >= 3:
        # leaving the frame on all four sides
        fwd[0, cols // 2] = (0.25, -2.5)
        fwd[rows - 1, cols // 2] = (-0.25, 2.5)
        fwd[rows // 2, 0] = (-2.5, 0.25)
        fwd[rows // 2, cols - 1] = (2.5, -0.25)
        notes["leaving"] = [(0, cols // 2), (rows - 1, cols // 2), (rows // 2, 0), (rows // 2, cols - 1)]
    if specials and rows >= 5 and cols >= 3:
        fwd[1, 1] = (np.nan, 0.5)
        fwd[3, 1] = (0.25, np.inf)
        fwd[1, 0] = (-np.inf, 0.0)
        notes["fwd_special"] = [(1, 1), (3, 1), (1, 0)]
        # a landing point exactly on the last column / row, answered by the backward field there: kept, with ax = 1 / ay = 1
        u = float(cols - 1)
        fwd[3, 0] = (u, 0.0)
        bwd[3, cols - 1] = (-u, 0.0)
        bwd[3, cols - 2] = (-u, 0.0)
        notes["on_last_column"] = (3, 0)
        # ... and one unit in the last place outside (column 0: j + u is exact): rejected
        fwd[4, 0] = (np.nextafter(float(cols - 1), np.inf), 0.0)
        notes["ulp_outside"] = (4, 0)
        if rows >= 16:
            v = float(rows - 1 - 9)
            fwd[9, 2] = (0.0, v)
            bwd[rows - 1, 2] = (0.0, -v)
            bwd[rows - 2, 2] = (0.0, -v)
            notes["on_last_row"] = (9, 2)
            # a NaN in one tap of the backward field rejects exactly the pixels that read it (those landing in the 2 x 2 cells around it)
            bwd[rows - 4, cols - 4, 1] = np.nan
            notes["bwd_nan"] = (rows - 4, cols - 4)
    return np.ascontiguousarray(fwd), np.ascontiguousarray(bwd), notes


def occluded_scene(synth, rows=96, cols=128):
    """the occluded pair of tests/test_flow_check_cpu.py and tests/test_gpu_flow_checked.py: (img1, img2, occluded, block plane, far background)"""
    gamma = 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = synth.default_motion()
    f0, _ = synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    s = 3.0 / np.abs(f0).max()
    y0, x0, h, bw, dx, dy = 30, 40, 28, 36, -8, 5
    img1, img2, occluded, block = synth.render_occluded_pair(rows, cols, K, v * s, w * s, k, gamma, seed=21, block=(y0, x0, h, bw), block_motion=(dx, dy))
    far = np.zeros((rows, cols), dtype=bool)
    far[9:rows - 9, 9:cols - 9] = True
    for yy, xx in ((y0, x0), (y0 + dy, x0 + dx)):
        far[max(0, yy - 8):yy + h + 8, max(0, xx - 8):xx + bw + 8] = False
    return img1, img2, occluded, block, far
