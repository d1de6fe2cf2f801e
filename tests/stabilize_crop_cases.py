"""Inputs of the crop's tests (tests/test_stabilize_crop_cpu.py, tests/test_gpu_stabilize_crop.py) and of its golden fixture
(tests/golden/make_golden_stabilize_crop.py): the masks whose windows are known exactly, the exact zoom-2 case on the stabiliser's shift
case, random masks, and the static scene's truth at a window's targets."""
import numpy as np

import stabilize_crop_spec_numpy as spec
import stabilize_spec_numpy as stab
from stabilize_fill_cases import POSE, clip_case, inputs, shift_case, shift_fill_case, static_scene  # noqa: F401  (reused as they are)

# tests/test_stabilize_crop_cpu.py::test_accuracy_against_the_analytic_truth, measured on the CPU (the spec on the neighbour's holed map, 3
# iterations, through the window the search finds on the filled frame's mask): the position error in pixels and the mean absolute error over
# the pixels the neighbour, rendered alone, offers, and the bounds the GPU-free test asserts, the measured values plus half of them
ACC_MEASURED = 0.265833
ACC_BOUND = 1.5 * ACC_MEASURED
ACC_MAE_MEASURED = 0.359596
ACC_MAE_BOUND = 1.5 * ACC_MAE_MEASURED

ZOOM2_WINDOW = (4, 14, 12, 20)  # on the shift case (24 x 40): a zoom of exactly 2 in both directions


def _ones(rows, cols, empty=()):
    m = np.ones((rows, cols), dtype=np.uint8)
    for r, c in empty:
        m[r, c] = 0
    return m


def _column(rows, cols, c):
    m = np.ones((rows, cols), dtype=np.uint8)
    m[:, c] = 0
    return m


def exact_windows():
    """-> list of (name, masks (planes, rows, cols) uint8, max_empty, margin, window): the windows a prototype of the definition gave"""
    shift = shift_case()["mask"]  # 24 x 40, set in rows 0 .. 19, columns 8 .. 39
    return [("shift-m0", shift[None], 0, 0, (1, 8, 19, 31)),
            ("shift-m1", shift[None], 0, 1, (0, 9, 19, 31)),
            ("7x5-full", _ones(7, 5)[None], 0, 0, (0, 0, 7, 5)),
            ("7x5-hole", _ones(7, 5, [(3, 2)])[None], 0, 0, (1, 0, 4, 2)),
            ("7x5-hole-allowed", _ones(7, 5, [(3, 2)])[None], 1, 0, (0, 0, 7, 5)),
            ("33x70-hole", _ones(33, 70, [(16, 35)])[None], 0, 0, (0, 18, 16, 33)),
            ("6x9-empty", np.zeros((1, 6, 9), dtype=np.uint8), 0, 0, (0, 0, 0, 0)),
            ("6x9-empty-allowed", np.zeros((1, 6, 9), dtype=np.uint8), 54, 0, (0, 0, 6, 9)),
            ("6x9-column", _column(6, 9, 4)[None], 0, 0, (1, 0, 3, 4))]  # a four-way tie


def random_masks(rows, cols, planes, empty, seed, set_value=1):
    """planes x rows x cols bytes, each pixel of each plane empty with probability `empty`"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((planes, rows, cols)) < empty, 0, set_value).astype(np.uint8)


def zoom2_case():
    """the shift case (D exactly (8, -4)) through ZOOM2_WINDOW: px = 6 + ix / 2 - 0.25, py = 8 + iy / 2 - 0.25 exactly, all inside the frame"""
    s = shift_case()
    rows, cols = s["depth"].shape
    iy, ix = np.mgrid[0:rows, 0:cols].astype(np.float64)
    return dict(s, window=ZOOM2_WINDOW, px=6.0 + ix / 2.0 - 0.25, py=8.0 + iy / 2.0 - 0.25)


def static_scene_window(synth, pose_table, window, rows=96, cols=128):
    """stabilize_fill_cases.static_scene plus the truth AT THE WINDOW'S TARGETS: frame 1's forward map on the TRUE depth into the virtual camera
    of frame 0, inverted by 50 fixed-point iterations about the targets (synth._bilinear: independent of stage C), and the texture there.
    -> static_scene's dict with truth_w (rows, cols, 3) float64, px_w, py_w and (Mn, mn), the neighbour's pose"""
    sc = static_scene(synth, pose_table, rows, cols)
    depth = synth.scene_depth(rows, cols)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    Mn, mn = sc["As"][0].T @ sc["A"][1], sc["As"][0].T @ (sc["c"][1] - sc["cs"][0])
    gx, gy, _ = stab.forward_map(depth, sc["Rs"][1], sc["ts"][1], *sc["K"], Mn, mn)
    F = np.stack([gx - xx, gy - yy], axis=-1)
    tx, ty = spec.window_targets(window, rows, cols)
    px, py = tx.copy(), ty.copy()
    for _ in range(50):
        d = synth._bilinear(F, px, py)
        px, py = tx - d[..., 0], ty - d[..., 1]
    return dict(sc, truth_w=synth._texture(px, py, 0x5EED0000), px_w=px, py_w=py, Mn=Mn, mn=mn)
