"""Inputs of the seam blend's tests (tests/test_stabilize_blend_cpu.py, tests/test_gpu_stabilize_blend.py) and of its golden fixture
(tests/golden/make_golden_stabilize_blend.py): masks for the distance, in-out planes and layers that drive the blend kernel's three paths, the
exposure case of the accuracy test."""
import numpy as np

import stabilize_blend_spec_numpy as spec
from stabilize_crop_cases import clip_case, random_masks  # noqa: F401  (reused as they are)

DISTANCE_SIZES = [(3, 5), (7, 5), (33, 70), (96, 128), (40, 1100), (2, 2)]  # the byte path, the byte tail, a row longer than one segment
FEATHERS = [1, 2, 16, 64]
ACC_GAINS = [0.8, 0.9, 1.1, 1.2]


def distance_masks(rows, cols, seed):
    """-> list of (name, mask): all set, all empty, one hole in a corner, one in the centre, random with 1 and with 255 as the set value"""
    ones = np.ones((rows, cols), dtype=np.uint8)
    corner, centre = ones.copy(), ones.copy()
    corner[rows - 1, 0] = 0
    centre[rows // 2, cols // 2] = 0
    return [("set", ones), ("empty", np.zeros_like(ones)), ("corner", corner), ("centre", centre),
            ("random-1", random_masks(rows, cols, 1, 0.02, seed, set_value=1)[0]), ("random-255", random_masks(rows, cols, 1, 0.3, seed + 1, set_value=255)[0])]


def brute_distance(mask, T):
    """the definition itself: per set pixel the chessboard distance to the nearest empty pixel of the frame, capped at T"""
    rows, cols = mask.shape
    ey, ex = np.nonzero(mask == 0)
    out = np.zeros((rows, cols), dtype=np.uint8)
    for y in range(rows):
        for x in range(cols):
            if mask[y, x] != 0:
                out[y, x] = T if ey.size == 0 else min(T, int(np.maximum(np.abs(ey - y), np.abs(ex - x)).min()))
    return out


def layer_case(rows, cols, ch, seed, T, sparse=False):
    """in-out planes and a layer with every combination inside one dword: an own frame whose mask is empty in a band on the left and at the
    top and in scattered holes, empty pixels a nearer candidate already took (source 2 or 3, mask 1), own pixels already blended (source 2),
    layer masks of 0, 1 and 255, and (unless sparse) a wide interior where the distance is T and every pixel is sourced: the untouched path.
    -> dict(image, mask, source, dist, layer, lmask)"""
    rng = np.random.default_rng(seed)
    shape = (rows, cols) if ch == 1 else (rows, cols, ch)
    own = np.ones((rows, cols), dtype=np.uint8)
    own[:max(rows // 6, 1)] = 0
    own[:, :max(cols // 5, 1)] = 0
    own[rng.random((rows, cols)) < (0.05 if sparse else 0.0003)] = 0
    dist = spec.seam_distance(own, T)
    source = own.copy()
    taken = (own == 0) & (rng.random((rows, cols)) < 0.3)
    source[taken] = rng.integers(2, 4, size=int(taken.sum()))
    done = (own == 1) & (rng.random((rows, cols)) < 0.05)
    source[done] = 2
    mask = (source != 0).astype(np.uint8)
    image = rng.integers(0, 256, size=shape, dtype=np.uint8)
    layer = rng.integers(0, 256, size=shape, dtype=np.uint8)
    lmask = rng.choice(np.array([0, 1, 255], dtype=np.uint8), size=(rows, cols), p=[0.2, 0.4, 0.4])
    return dict(image=image, mask=mask, source=source, dist=dist, layer=layer, lmask=lmask)


def exposure_case(g, rows=96, cols=128, T=16):
    """the accuracy test's input: a smooth texture in [6, 200] as the own frame, empty in a band of 24 columns, and the same texture times g,
    rounded, as a layer that covers the frame.  -> dict(texture float64, image, mask, source, dist, layer, lmask)"""
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    texture = 103.0 + 60.0 * np.sin(xx / 17.0 + 0.3) * np.cos(yy / 13.0) + 37.0 * np.sin((xx + 2.0 * yy) / 29.0)  # in [6, 200]
    assert texture.min() >= 6.0 and texture.max() <= 200.0
    mask = np.ones((rows, cols), dtype=np.uint8)
    mask[:, 40:64] = 0
    image = np.where(mask == 1, np.rint(texture), 0).astype(np.uint8)
    layer = np.rint(g * texture).astype(np.uint8)  # at most 240: nothing saturates
    return dict(texture=texture, image=image, mask=mask, source=mask.copy(), dist=spec.seam_distance(mask, T), layer=layer, lmask=np.ones_like(mask), T=T)
