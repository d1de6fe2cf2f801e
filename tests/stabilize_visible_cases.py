"""Inputs of the occlusion test's tests (tests/test_stabilize_visible_cpu.py, tests/test_gpu_stabilize_visible.py) and of its golden fixture
(tests/golden/make_golden_stabilize_visible.py): the fold scene -- a fronto-parallel box in front of a far background, seen from a camera
moved sideways, the smallest scene whose map folds -- at the smallest shapes where the kernels can go wrong, and the dense rectifier's
inputs (tests/rectify_dense_cases.py) for the paths the fold scene does not reach."""
import numpy as np

import link_spec_numpy as link
import stabilize_visible_spec_numpy as spec
from rectify_dense_cases import POSE, inputs  # noqa: F401  (reused as they are)

Z_BOX, Z_BACK, FX, SHIFT = 2.0, 10.0, 40.0, 0.6  # disparities 12 and 2.4 pixels: a fold band of 9.6
FOLD_SHAPES = [(24, 40), (37, 67), (16, 131)]    # 37 x 67: 2479 pixels, a 3-pixel byte tail, 3 workgroups; 16 x 131: three column tiles, one ragged
M_N = link.rodrigues(np.array([-0.03, 0.04, -0.02]))  # tests/test_gpu_stabilize_fill.py's neighbour pose
m_N = np.array([-0.1, 0.05, -0.15])
SID = 2


def box_of(rows, cols):
    """(r0, r1, c0, c1) of the box in the SOURCE frame: 13 columns from either edge at least, so that its footprint stays in the frame"""
    return rows // 4, rows - rows // 4, max(13, (3 * cols) // 10), min(cols - 13, (7 * cols) // 10)


def footprint_of(rows, cols, sign, erode=2):
    """the box's analytic footprint in the virtual camera moved by sign * SHIFT, eroded: (r0, r1, c0, c1), integers"""
    r0, r1, c0, c1 = box_of(rows, cols)
    d = int(round(sign * SHIFT * FX / Z_BOX))  # 12 pixels, exactly
    return r0 + erode, r1 - erode, c0 - d + erode, c1 - d - erode


def _planes(rows, cols, channels, seed):
    """the in-out planes a call starts from: random bytes, so that "keeps what it had" shows"""
    rng = np.random.default_rng(seed)
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    return rng.integers(0, 256, size=shape, dtype=np.uint8), rng.integers(6, 200, size=(rows, cols), dtype=np.uint8)


def _case(name, image, depth, R, t, K, M, m, window=None, mask0=None, tol_q16=0, mode=0, q5_mode=0, iterations=0):
    rows, cols = depth.shape
    image0, source0 = _planes(rows, cols, 1 if image.ndim == 2 else 3, rows * 131 + cols)
    return dict(name=name, image=image, depth=depth, R=R, t=t, K=K, M=np.asarray(M, dtype=np.float64), m=np.asarray(m, dtype=np.float64),
                window=tuple(window) if window else (0, 0, rows, cols), mask0=np.zeros((rows, cols), dtype=np.uint8) if mask0 is None else mask0, image0=image0,
                source0=source0, tol_q16=tol_q16, mode=mode, q5_mode=q5_mode, iterations=iterations)


def fold_case(rows, cols, channels=3, sign=1, window=None, mask0=None, name=None, tol_q16=0):
    """the box (values 160 .. 255) over the background (values 0 .. 95), identity pose tables, the virtual camera moved by sign * SHIFT
    along x: a point X of the source is X - (sign SHIFT, 0, 0) in it"""
    rng = np.random.default_rng(rows * 1000 + cols)
    r0, r1, c0, c1 = box_of(rows, cols)
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    image = rng.integers(0, 96, size=shape, dtype=np.uint8)
    image[r0:r1, c0:c1] = rng.integers(160, 256, size=image[r0:r1, c0:c1].shape, dtype=np.uint8)
    depth = np.full((rows, cols), Z_BACK)
    depth[r0:r1, c0:c1] = Z_BOX
    R, t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
    K = (FX, FX, cols / 2.0, rows / 2.0)
    name = name or "fold-%dx%d-%s-%s" % (rows, cols, "bgr" if channels == 3 else "gray", "plus" if sign > 0 else "minus")
    return _case(name, image, depth, R, t, K, np.eye(3), (-sign * SHIFT, 0.0, 0.0), window, mask0, tol_q16)


def pattern_mask(rows, cols):
    """every pattern of the 4 bytes of a word, and whole words set"""
    i = np.arange(rows * cols)
    return ((i // 4 % 16) >> (i % 4) & 1).astype(np.uint8).reshape(rows, cols)


def dense_case(pose_table, name, rows, cols, channels=3, M=M_N, m=m_N, mask0=None, **kw):
    """the dense rectifier's inputs with its rolling-shutter pose table (pose_table: oracle_py's), seen with (M, m)"""
    K, image, depth = inputs(rows, cols, channels=channels, **kw)
    R, t = pose_table(POSE["v"], POSE["w"], POSE["k"], POSE["gamma"], rows)
    return _case(name, image, depth, np.ascontiguousarray(R).reshape(rows, 9), np.asarray(t, dtype=np.float64), K, M, m, mask0=mask0)


def all_cases(pose_table):
    """-> list of case dicts, names unique"""
    out = [fold_case(r, c, ch, sign) for r, c in FOLD_SHAPES for ch, sign in ((3, 1), (1, -1), (3, -1), (1, 1))]
    rows, cols = 37, 67
    h = rows - 5
    out.append(fold_case(rows, cols, 3, 1, window=(2, 3, h, (h * cols) // rows), name="fold-zoom"))
    out.append(fold_case(rows, cols, 3, -1, mask0=pattern_mask(rows, cols), name="fold-partial-mask"))
    out.append(fold_case(rows, cols, 1, 1, tol_q16=65536, name="fold-tol-max"))
    out.append(dense_case(pose_table, "rs-table", 33, 70, holes=0.0))
    out.append(dense_case(pose_table, "holes", 33, 70, channels=1, holes=0.4, mask0=pattern_mask(33, 70)))
    out.append(dense_case(pose_table, "2x2", 2, 2, holes=0.0))
    out.append(dense_case(pose_table, "no-valid-depth", 33, 70, none_valid=True))
    out.append(dense_case(pose_table, "many-to-one", 37, 67, holes=0.0, M=np.eye(3), m=(0.0, 0.0, 30.0)))
    assert len({c["name"] for c in out}) == len(out)
    return out


def run_spec(case, visible=True):
    """the definition on a case's planes.  -> dict(image, mask, source, counts (taken, rejected)); visible=False: the plain window fill, rejected 0"""
    out, mask, source = case["image0"].copy(), case["mask0"].copy(), case["source0"].copy()
    args = (out, mask, source, case["image"], case["depth"], case["R"], case["t"], case["K"], case["M"], case["m"], SID, case["window"])
    kw = dict(mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    counts = spec.fill_from_visible(*args, tol_q16=case["tol_q16"], **kw) if visible else (spec.crop.fill_from_window(*args, **kw), 0)
    return dict(image=out, mask=mask, source=source, counts=tuple(int(x) for x in counts))


def random_case(seed):
    """a tiny frame drawn from `seed`: rows, cols in 2 .. 70, a smooth depth plus a box nearer the camera, a small pose, a random pre-set mask"""
    rng = np.random.default_rng(seed)
    rows, cols = int(rng.integers(2, 71)), int(rng.integers(2, 71))
    channels = 3 if rng.random() < 0.5 else 1
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    depth = 6.0 + 2.0 * np.sin(x / 9.0 + rng.random()) * np.cos(y / 7.0 + rng.random())
    r0, c0 = int(rng.integers(0, rows)), int(rng.integers(0, cols))
    depth[r0:r0 + int(rng.integers(1, rows + 1)), c0:c0 + int(rng.integers(1, cols + 1))] = rng.uniform(1.0, 3.0)
    image = rng.integers(0, 256, size=(rows, cols) if channels == 1 else (rows, cols, 3), dtype=np.uint8)
    R, t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
    K = (float(rng.uniform(20.0, 60.0)),) * 2 + (cols / 2.0 - 0.3, rows / 2.0 + 0.2)
    M, m = link.rodrigues(rng.normal(size=3) * 0.02), rng.normal(size=3) * np.array([0.4, 0.4, 0.2])
    mask0 = (rng.random((rows, cols)) < rng.random()).astype(np.uint8)
    return _case("random-%d" % seed, image, depth, R, t, K, M, m, mask0=mask0, iterations=int(rng.integers(0, 4)))
