"""Inputs of the visible pre-image search's tests (tests/test_stabilize_search_cpu.py, tests/test_gpu_stabilize_search.py) and of its golden
fixture (tests/golden/make_golden_stabilize_search.py): every case of tests/stabilize_visible_cases.py, reused as it is, and two of its own --
a fold of two layers, and a fold seen through a zoom window with ONE iteration from a camera that also moved back, where several source
pixels of one depth land on one cell and the key's tie-break decides where the restart begins."""
import numpy as np

import stabilize_search_spec_numpy as spec
import stabilize_visible_cases as vcases
from stabilize_visible_cases import FOLD_SHAPES, SID, fold_case, footprint_of, pattern_mask, random_case  # noqa: F401  (reused as they are)

Z_MID = 4.0
TIE_CASE = "fold-zoom-once"


def two_layer_case(rows=37, cols=67, channels=3, sign=1):
    """boxes at z = 2 (values 176 .. 255) and, 3 rows and 6 columns wider on every side, z = 4 (values 96 .. 143) over the background at z = 10
    (values 0 .. 63): two folds, one behind the other"""
    rng = np.random.default_rng(rows * 977 + cols)
    r0, r1, c0, c1 = vcases.box_of(rows, cols)
    m0, m1, n0, n1 = max(r0 - 3, 0), min(r1 + 3, rows), max(c0 - 6, 0), min(c1 + 6, cols)
    image = rng.integers(0, 64, size=(rows, cols) if channels == 1 else (rows, cols, 3), dtype=np.uint8)
    depth = np.full((rows, cols), vcases.Z_BACK)
    image[m0:m1, n0:n1] = rng.integers(96, 144, size=image[m0:m1, n0:n1].shape, dtype=np.uint8)
    depth[m0:m1, n0:n1] = Z_MID
    image[r0:r1, c0:c1] = rng.integers(176, 256, size=image[r0:r1, c0:c1].shape, dtype=np.uint8)
    depth[r0:r1, c0:c1] = vcases.Z_BOX
    R, t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
    return vcases._case("two-layer", image, depth, R, t, (vcases.FX, vcases.FX, cols / 2.0, rows / 2.0), np.eye(3), (-sign * vcases.SHIFT, 0.0, 0.0))


def zoom_once_case(rows=24, cols=40):
    """the fold through a zoom window with iterations = 1, the virtual camera also moved BACK by 0.5: the image shrinks, several source pixels of
    one depth share a cell, and with a single step the restart's end depends on where it began -- the tie rule shows in the bytes"""
    h = rows - 5
    case = fold_case(rows, cols, 3, 1, window=(2, 3, h, (h * cols) // rows), name=TIE_CASE)
    case["m"] = np.array([-vcases.SHIFT, 0.0, 0.5])
    case["iterations"] = 1
    return case


def all_cases(pose_table):
    """-> list of case dicts, names unique: the occlusion test's cases and the two above"""
    out = vcases.all_cases(pose_table) + [two_layer_case(), zoom_once_case()]
    assert len({c["name"] for c in out}) == len(out)
    return out


def run_spec(case, _largest_index=False):
    """the definition on a case's planes.  -> dict(image, mask, source, counts (taken, rejected, recovered))"""
    out, mask, source = case["image0"].copy(), case["mask0"].copy(), case["source0"].copy()
    counts = spec.fill_from_search(out, mask, source, case["image"], case["depth"], case["R"], case["t"], case["K"], case["M"], case["m"], SID, case["window"],
                                   tol_q16=case["tol_q16"], mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"], _largest_index=_largest_index)
    return dict(image=out, mask=mask, source=source, counts=tuple(int(x) for x in counts))


def run_visible(case):
    """the occlusion test's definition on the same planes.  -> dict(image, mask, source, counts (taken, rejected))"""
    return vcases.run_spec(case)
