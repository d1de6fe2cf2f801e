"""Inputs of the inpainting's tests (tests/test_stabilize_inpaint_cpu.py, tests/test_gpu_stabilize_inpaint.py) and of its golden fixture
(tests/golden/make_golden_stabilize_inpaint.py): the sizes, the mask families, a second formulation of the definition in plain loops over
cells, and the accuracy test's holes."""
import numpy as np

import stabilize_inpaint_spec_numpy as spec
from stabilize_blend_cases import exposure_case

CPU_SIZES = [(2, 2), (3, 5), (7, 5), (33, 70), (129, 67)]
# (3, 5), (7, 5), (33, 70), (401, 603): rows that do not start on a dword; (129, 67), (401, 603): odd at every level; (2, 4099): one row of
# cells; (401, 603): the smallest frame with a large pull, the single-workgroup launch and two large pushes (6 launches)
GPU_SIZES = CPU_SIZES + [(2, 4099), (401, 603)]
ACC_HOLES = [("rows 30-49 x cols 60-89", (slice(30, 50), slice(60, 90))), ("rows 40-47 x cols 20-27", (slice(40, 48), slice(20, 28))),
             ("cols 0-11", (slice(None), slice(0, 12))), ("cols 40-63", (slice(None), slice(40, 64)))]


def image_of(rows, cols, ch, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(rows, cols) if ch == 1 else (rows, cols, ch), dtype=np.uint8)


def masks(rows, cols, seed):
    """-> list of (name, mask): all set, all empty, only the last pixel set, bands at the left and top plus scattered holes, random with 30 %
    set and 255 as the set value"""
    rng = np.random.default_rng(seed)
    ones = np.ones((rows, cols), dtype=np.uint8)
    last = np.zeros_like(ones)
    last[rows - 1, cols - 1] = 1
    bands = ones.copy()
    bands[:max(rows // 6, 1)] = 0
    bands[:, :max(cols // 5, 1)] = 0
    bands[rng.random((rows, cols)) < 0.05] = 0
    sparse = np.where(rng.random((rows, cols)) < 0.3, 255, 0).astype(np.uint8)
    return [("set", ones), ("empty", np.zeros_like(ones)), ("last", last), ("bands", bands), ("random-255", sparse)]


def big_hole(rows, cols, seed):
    """a 150 x 200 hole (cells stay invalid several levels up) in a frame with scattered holes"""
    m = masks(rows, cols, seed)[3][1].copy()
    m[rows // 3:rows // 3 + 150, cols // 4:cols // 4 + 200] = 0
    return m


def loop_inpaint(image, mask, source=None):
    """the definition once more, cell by cell in plain Python integers: nothing shared with the spec's vectorised code"""
    rows, cols = mask.shape
    ch = 1 if image.ndim == 2 else image.shape[2]
    px = image.reshape(rows, cols, ch)
    level = [[([int(px[y, x, c]) << 8 for c in range(ch)] if mask[y, x] != 0 else None) for x in range(cols)] for y in range(rows)]
    levels = [level]
    while len(level) > 1 or len(level[0]) > 1:
        h, w = len(level), len(level[0])
        up = []
        for Y in range((h + 1) // 2):
            row = []
            for X in range((w + 1) // 2):
                kids = [level[y][x] for y in (2 * Y, 2 * Y + 1) for x in (2 * X, 2 * X + 1) if y < h and x < w and level[y][x] is not None]
                n = len(kids)
                row.append([(sum(k[c] for k in kids) + (n >> 1)) // n for c in range(ch)] if n else None)
            up.append(row)
        levels.append(up)
        level = up
    if levels[-1][0][0] is None:
        return 0
    far = lambda i, n: min(max((i >> 1) + (1 if i & 1 else -1), 0), n - 1)
    for l in range(len(levels) - 2, -1, -1):
        fine, coarse = levels[l], levels[l + 1]
        hc, wc = len(coarse), len(coarse[0])
        for y in range(len(fine)):
            for x in range(len(fine[0])):
                if fine[y][x] is None:
                    yn, xn, yf, xf = y >> 1, x >> 1, far(y, hc), far(x, wc)
                    fine[y][x] = [(9 * coarse[yn][xn][c] + 3 * coarse[yn][xf][c] + 3 * coarse[yf][xn][c] + coarse[yf][xf][c] + 8) >> 4 for c in range(ch)]
    count = 0
    for y in range(rows):
        for x in range(cols):
            if mask[y, x] == 0:
                for c in range(ch):
                    px[y, x, c] = (levels[0][y][x][c] + 128) >> 8
                if source is not None:
                    source[y, x] = spec.SOURCE_INPAINTED
                count += 1
    return count


def accuracy_case(hole):
    """the blend's exposure texture at 96 x 128 with `hole` (a pair of slices) empty -> (texture float64, image, mask)"""
    e = exposure_case(1.0)
    mask = np.ones((96, 128), dtype=np.uint8)
    mask[hole] = 0
    image = np.where(mask == 1, np.rint(e["texture"]), 0).astype(np.uint8)
    return e["texture"], image, mask
