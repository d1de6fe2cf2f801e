"""Inputs of the dense rectifier's tests (tests/test_rectify_dense_cpu.py, tests/test_gpu_rectify_dense.py) and of its golden fixture
(tests/golden/make_golden_rectify_dense.py): the images, camera and pose of tests/test_gpu_rectify_gray.py (_inputs), with a THINNED depth map."""
import numpy as np

POSE = dict(v=np.array([0.3, -0.2, 0.1]), w=np.array([0.02, 0.03, -0.04]), k=0.1, gamma=0.9)  # tests/test_gpu_rectify_gray.py::_oracle


def camera(rows, cols):
    return (0.8 * cols, 0.8 * cols, cols / 2.0 - 0.3, rows / 2.0 + 0.2)


def inputs(rows, cols, channels=3, holes=0.4, block=None, corner=None, specials=False, none_valid=False):
    """K, image (rows, cols[, 3]) uint8 and depth (rows, cols): test_gpu_rectify_gray._inputs' gray image (2 % marker pixels, 5 % values 0..8;
    two more random channels for BGR) and its depth map uniform in [0.6, 2.5] with a fraction `holes` of it zeroed at random, a block
    (y0, x0, h, w) and a corner block (h, w) zeroed on top.  specials: NaN, inf, negative and 1e308 depths among the valid ones.
    none_valid: nothing but zeros, NaN, inf and negative values."""
    rng = np.random.default_rng(rows * 7 + cols)
    g = rng.integers(16, 256, size=(rows, cols), dtype=np.uint8)
    g[rng.random((rows, cols)) < 0.02] = 1
    dark = rng.random((rows, cols)) < 0.05
    g[dark] = rng.integers(0, 9, size=int(dark.sum()), dtype=np.uint8)
    depth = rng.uniform(0.6, 2.5, size=(rows, cols))
    image = g if channels == 1 else np.ascontiguousarray(np.stack([g, rng.integers(0, 256, size=(rows, cols), dtype=np.uint8),
                                                                   rng.integers(0, 256, size=(rows, cols), dtype=np.uint8)], axis=-1))
    depth[rng.random((rows, cols)) < holes] = 0.0
    if block:
        y0, x0, h, w = block
        depth[y0:y0 + h, x0:x0 + w] = 0.0
    if corner:
        depth[rows - corner[0]:, cols - corner[1]:] = 0.0
    if specials or none_valid:
        flat = depth.reshape(-1)
        idx = rng.permutation(flat.size)[:max(4, flat.size // 10)]
        vals = [np.nan, np.inf, -np.inf, -1.5, 0.0] if none_valid else [np.nan, np.inf, -np.inf, -1.5, 1e308]
        if none_valid:
            flat[:] = 0.0
        flat[idx] = np.resize(vals, idx.size)
    return camera(rows, cols), image, depth
