"""Inputs of the last-frame tests (tests/last_frame_spec_numpy.py is the definition): the families the GPU test holds the advance to bit for
bit, built on the link's and the fusion's generators; a second formulation of the advance in plain loops over pixels; and the coverage scene."""
import numpy as np

import fuse_cases
import link_cases

# the edges of the 64 x 16 LDS tile and of a wave: smaller than a tile, exactly one, ragged both ways, several workgroups
SHAPES = [(2, 2), (3, 5), (16, 64), (17, 33), (65, 130), (96, 128), (300, 400)]
CPU_SHAPES = [(2, 2), (3, 5), (16, 64), (17, 33), (65, 130)]
KS = (0.0, 0.3, -0.3)
FAMILIES = ("model", "one_pixel", "leaving", "bad_vectors", "bad_depths", "empty")
COVERAGE_BOUND = 0.80  # of the frame, and of the pixels the map holds (the spec gives 0.951 and 0.956: tests/test_last_frame_cpu.py)


def family(name, rows, cols, k=0.2):
    """-> dict(F, Z, v, w, k, K, gamma)"""
    d = link_cases.base_case(rows, cols, 0.3, salt=31)
    F, Z = d["F"], d["Zp"]
    r = np.random.default_rng(97 * rows + cols)
    if name == "model":
        pass
    elif name == "one_pixel":  # every vector points at one pixel: rows * cols offers to it, holes aside
        ii, jj = np.mgrid[0:rows, 0:cols].astype(np.float64)
        ti, tj = rows // 2, cols // 3
        F[..., 0], F[..., 1] = tj - jj + r.uniform(-0.4, 0.4, (rows, cols)), ti - ii + r.uniform(-0.4, 0.4, (rows, cols))
        F[ti, tj] = (0.25, -0.25)  # (0, 0) would not be usable
    elif name == "leaving":  # a third stays, the rest leaves through every border, some by far
        pick = r.integers(0, 6, (rows, cols))
        F[pick == 1] = (float(cols), 0.3)
        F[pick == 2] = (-float(cols) - 0.51, 0.0)
        F[pick == 3] = (0.2, float(rows) + 0.5)
        F[pick == 4] = (1e300, -1e300)
        F[0, 0], F[rows - 1, cols - 1] = (-0.5, -0.5), (0.49, 0.49)  # on the first pixel exactly, half a pixel short of leaving
        Z[0, 0] = Z[rows - 1, cols - 1] = 1.25
    elif name == "bad_vectors":
        vals = np.array([[0.0, 0.0], [-0.0, 0.0], [np.nan, 1.0], [1.0, np.nan], [np.inf, 0.0], [0.0, -np.inf], [np.nan, np.nan], [0.5, -0.5]])
        F[:] = vals[r.integers(0, len(vals), (rows, cols))]
        Z[:] = 1.0 + r.uniform(0, 1, (rows, cols))
    elif name == "bad_depths":
        vals = np.array([np.nan, np.inf, -np.inf, -1.5, 0.0, -0.0, 5e-324, 2.2e-308, 1e308, 1.0, 0.75])
        Z[:] = vals[r.integers(0, len(vals), (rows, cols))]
    elif name == "empty":
        Z[:] = link_cases.empty_case(rows, cols)["Zp"]
    else:
        raise KeyError(name)
    return dict(F=np.ascontiguousarray(F), Z=np.ascontiguousarray(Z), v=d["v"], w=d["w"], k=float(k), K=d["K"], gamma=d["gamma"])


def loop_advance(F, Z, v, w, k, K, gamma, global_shutter=False, order=None):
    """the advance pixel by pixel with Python floats (IEEE doubles, one rounding per operation), a float z-buffer instead of the integer one.
    order: a permutation of the pixels (the offers' order must not matter).  -> (map, count)"""
    import math

    rows, cols = Z.shape
    fx, fy, cx, cy = (float(x) for x in K)
    gamma, k, h = float(gamma), float(k), float(rows)
    v2, w0, w1 = float(v[2]), float(w[0]), float(w[1])
    out = [[None] * cols for _ in range(rows)]
    ok = lambda z: z > 0.0 and z < math.inf
    for n in (range(rows * cols) if order is None else order):
        i, j = divmod(int(n), cols)
        z, fu, fv = float(Z[i, j]), float(F[i, j, 0]), float(F[i, j, 1])
        if not ok(z) or not (math.isfinite(fu) and math.isfinite(fv)) or (fu == 0.0 and fv == 0.0):
            continue
        qx, qy = (j - cx) * 1.0 / fx, (i - cy) * 1.0 / fy
        alpha = 1.0 if global_shutter else 1 + gamma * fv / h
        part1, part2 = gamma * i / h, 1.0 + gamma * (i + fv) / h
        alpha_k = 0.5 * (part2 * part2 - part1 * part1)
        b = ((2.0 * (alpha + k * alpha_k)) / (2.0 + k)) / gamma
        z_pred = z * (1.0 + b * (w0 * qy - w1 * qx)) + b * v2
        r2, c2 = math.floor((i + fv) + 0.5), math.floor((j + fu) + 0.5)
        if not (0 <= r2 <= rows - 1 and 0 <= c2 <= cols - 1) or not ok(z_pred):
            continue
        if out[r2][c2] is None or z_pred < out[r2][c2]:
            out[r2][c2] = z_pred
    count = sum(x is not None for row in out for x in row)
    return np.array([[0.0 if x is None else x for x in row] for row in out], dtype=np.float64), count


def coverage_scene(synth):
    """synth.make_flow at 96 x 128, K = (96, 96, 64, 48), the default motion scaled to a largest flow component of 3 px, gamma 0.8; the true
    depth, and the same with 30 % of it zeroed.  -> dict(F, Z, Z_holed, v, w, k, K, gamma)"""
    rows, cols, K, gamma = 96, 128, (96.0, 96.0, 64.0, 48.0), 0.8
    v, w, k = synth.default_motion()
    f0, _ = synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    s = 3.0 / np.abs(f0).max()
    F, truth = synth.make_flow(rows, cols, K, v * s, w * s, k, gamma, _model_only=True)
    Z = truth["Z"].copy()
    holed = Z.copy()
    holed[np.random.default_rng(7).random(Z.shape) < 0.30] = 0.0
    return dict(F=F, Z=Z, Z_holed=holed, v=v * s, w=w * s, k=k, K=K, gamma=gamma)
