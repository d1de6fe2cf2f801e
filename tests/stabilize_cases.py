"""Inputs of the stabiliser's tests (tests/test_stabilize_cpu.py, tests/test_gpu_stabilize.py) and of its golden fixture
(tests/golden/make_golden_stabilize.py): the dense rectifier's images, camera, pose and thinned depth maps (tests/rectify_dense_cases.py)
with one standard virtual pose, the exact shift case, and the paths the smoother is tested on."""
import numpy as np

import link_spec_numpy as link
import rectify_dense_cases as dense_cases
from rectify_dense_cases import POSE, camera, inputs  # noqa: F401  (reused as they are)

# the standard virtual pose: a small rotation and a translation in the pair's own unit (depths are 0.6 .. 2.5)
M_STD = link.rodrigues(np.array([0.01, -0.015, 0.02]))
m_STD = np.array([0.05, -0.03, 0.02])
M_ID, m_ID = np.eye(3), np.zeros(3)

# tests/test_stabilize_cpu.py::test_accuracy_against_the_analytic_truth, measured on the CPU (the spec on the holed map, 3 iterations):
# the position error in pixels and the bound the GPU-free test asserts, the measured value plus half of it
ACC_MEASURED = 0.289054
ACC_BOUND = 1.5 * ACC_MEASURED


def shift_case():
    """constant depth 4, identity pose table, K = (32, 32, 20, 12), M = I, m = (1, -0.5, 0) at 24 x 40: D is exactly (8, -4) everywhere, the
    output is the input shifted by (8, -4) and the mask is the in-frame region, 640 of 960 pixels"""
    rows, cols = 24, 40
    rng = np.random.default_rng(2440)
    image = rng.integers(0, 256, size=(rows, cols, 3), dtype=np.uint8)
    depth = np.full((rows, cols), 4.0)
    R, t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
    want = np.zeros_like(image)
    mask = np.zeros((rows, cols), dtype=np.uint8)
    want[:rows - 4, 8:] = image[4:, :cols - 8]  # output g samples the frame at p = g - (8, -4)
    mask[:rows - 4, 8:] = 1
    return dict(image=image, depth=depth, R=R, t=t, K=(32.0, 32.0, 20.0, 12.0), M=np.eye(3), m=np.array([1.0, -0.5, 0.0]), want=want, mask=mask, valid=640)


def uniform_path(F, w=(0.004, 0.01, -0.003), step=(0.02, -0.01, 0.05)):
    """uniform rotation about a fixed axis plus a straight walk: A_q = exp(q [w]x), c_q = q step"""
    w, step = np.asarray(w, dtype=np.float64), np.asarray(step, dtype=np.float64)
    A = np.stack([link.rodrigues(q * w) for q in range(F)])
    c = np.stack([q * step for q in range(F)])
    return A, c


def jitter_path(F, rot=0.01, pos=0.03, axis=(0.6, -0.64, 0.48), direction=(0.0, 0.6, 0.8)):
    """uniform_path with alternating +- rot rad about `axis` and +- pos units along `direction` on top"""
    A, c = uniform_path(F)
    axis, direction = np.asarray(axis, dtype=np.float64), np.asarray(direction, dtype=np.float64)
    Aj = np.stack([A[q] @ link.rodrigues((rot if q % 2 == 0 else -rot) * axis) for q in range(F)])
    cj = np.stack([c[q] + (pos if q % 2 == 0 else -pos) * direction for q in range(F)])
    return A, c, Aj, cj


def golden_path():
    """the 12-frame path of the golden fixture: a chain (tests/link_spec_numpy.py) of 11 pairs with varying motions and ratios, one link
    broken"""
    rng = np.random.default_rng(12)
    n, gamma = 11, 0.9
    vs = rng.normal(size=(n, 3)) * 0.1 + np.array([0.3, -0.2, 0.1])
    ws = rng.normal(size=(n, 3)) * 0.02
    ratios = rng.uniform(0.7, 1.4, size=n - 1)
    valids = np.ones(n - 1, dtype=bool)
    valids[4] = False
    ch = link.chain(ratios, valids, vs, ws, gamma)
    return dict(A=ch["A"], c=ch["c"], scales=ch["scales"], sigma=1.5, radius=0)


assert dense_cases.POSE is POSE
