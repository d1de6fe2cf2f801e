"""Inputs of the link tests (tests/link_spec_numpy.py is the definition): the cases the GPU test holds the kernels to bit for bit, and the
three-pair accuracy scene that the CPU test measures through the oracle and the GPU test repeats through the library's solve."""
import numpy as np

SHAPES = [(2, 2), (3, 5), (17, 70), (64, 64), (65, 129), (150, 200)]  # the edges of the 64 x 16 LDS tile and of a wave
HOLES = [0.0, 0.3, 0.97]
GAMMA = 0.8


def camera(rows, cols):
    return (0.75 * cols, 0.75 * cols, 0.5 * cols - 0.25, 0.5 * rows + 0.125)


def _rng(rows, cols, salt):
    return np.random.default_rng(1000003 * rows + 1009 * cols + salt)


def base_case(rows, cols, holes=0.3, salt=0):
    """a smooth field of a few pixels and two depth maps around 1 with the given share of holes (exact zeros, as the solve leaves pixels
    without an inlier); motion of the solve's size.  -> dict(F, Zp, Zn, v, w, k, K, gamma)"""
    r = _rng(rows, cols, salt)
    ii, jj = np.mgrid[0:rows, 0:cols].astype(np.float64)
    F = np.stack([2.5 * np.sin(0.11 * ii + 0.07 * jj) + r.normal(0, 0.3, (rows, cols)), 1.5 * np.cos(0.05 * ii - 0.09 * jj) + r.normal(0, 0.3, (rows, cols))], -1)
    Zp = 1.0 + 0.3 * np.sin(0.2 * ii) * np.cos(0.13 * jj) + r.uniform(0, 0.05, (rows, cols))
    Zn = 1.7 * (1.0 + 0.3 * np.sin(0.2 * ii + 0.1) * np.cos(0.13 * jj)) * np.exp(r.normal(0, 0.05, (rows, cols)))
    Zp[r.uniform(size=(rows, cols)) < holes] = 0.0
    Zn[r.uniform(size=(rows, cols)) < holes] = 0.0
    return dict(F=np.ascontiguousarray(F), Zp=Zp, Zn=Zn, v=np.array([0.6, -0.3, 0.74]) * 0.05, w=np.array([0.004, -0.006, 0.009]), k=0.2, K=camera(rows, cols),
                gamma=GAMMA)


def special_case(rows, cols):
    """base_case with 30 % holes plus, where the frame has room: NaN and +-inf depths in both maps, a negative depth, NaN / inf vectors, vectors
    that land outside every border, vectors that land exactly on the last row and column, and one half a pixel short of leaving"""
    d = base_case(rows, cols, 0.3, salt=7)
    F, Zp, Zn = d["F"], d["Zp"], d["Zn"]
    notes = {}
    if rows >= 16 and cols >= 16:
        for a, (i, j) in enumerate([(1, 1), (2, 3), (3, 5), (4, 7)]):
            Zp[i, j] = (np.nan, np.inf, -np.inf, -1.5)[a]
        for a, (i, j) in enumerate([(5, 2), (6, 4), (7, 6), (8, 8)]):
            Zn[i, j] = (np.nan, np.inf, -np.inf, -0.5)[a]
        F[9, 1] = (np.nan, 0.0)
        F[9, 3] = (0.0, np.inf)
        F[9, 5] = (-np.inf, np.nan)
        Zp[9, 1] = Zp[9, 3] = Zp[9, 5] = 1.0
        out = [(0, 4, (0.0, -0.75)), (rows - 1, 4, (0.0, 0.5)), (5, 0, (-0.51, 0.0)), (5, cols - 1, (0.5, 0.0)), (10, 10, (1e300, 0.0)), (11, 10, (0.0, -1e300))]
        for i, j, f in out:
            F[i, j], Zp[i, j] = f, 1.0
        notes["outside"] = [(i, j) for i, j, _ in out]
        on = [(3, 9, (float(cols - 1 - 9), 0.0)), (4, 9, (0.0, float(rows - 1 - 4))), (6, 11, (cols - 1 - 11 + 0.49, rows - 1 - 6 + 0.49)), (0, 0, (-0.5, -0.5))]
        for i, j, f in on:
            F[i, j], Zp[i, j] = f, 1.0
        Zn[rows - 1, :], Zn[:, cols - 1], Zn[0, 0], Zn[3, cols - 1] = 2.0, 2.0, 2.0, 2.0
        notes["on_border"] = [(i, j) for i, j, _ in on]
    return d, notes


def negative_prediction_case(rows, cols):
    """a strong v2 < 0: z_pred = z (1 + ...) + b v2 is negative for the nearer half of the scene"""
    d = base_case(rows, cols, 0.0, salt=11)
    d["v"] = np.array([0.0, 0.0, -0.9])
    return d


def empty_case(rows, cols):
    """no valid pixel at all: zeros, NaN, infinities and negative depths"""
    d = base_case(rows, cols, 0.0, salt=13)
    r = _rng(rows, cols, 14)
    d["Zp"] = r.choice(np.array([0.0, np.nan, np.inf, -np.inf, -2.0]), size=(rows, cols))
    return d


def planted_case(rows, cols, values, share=0.6, salt=17):
    """planes with planted ratios: Z_p = 1 with zero flow, v2 = 0 and w = (0, 0, wz) give z_pred = 1 exactly, so the ratio at a pixel is
    Z_n there, exactly.  `values`: the ratios to draw from (uniformly); `share`: the share of pixels that carry one"""
    r = _rng(rows, cols, salt)
    Zn = r.choice(np.asarray(values, dtype=np.float64), size=(rows, cols))
    Zn[r.uniform(size=(rows, cols)) >= share] = 0.0
    return dict(F=np.zeros((rows, cols, 2)), Zp=np.ones((rows, cols)), Zn=Zn, v=np.array([0.02, 0.01, 0.0]), w=np.array([0.0, 0.0, 0.01]), k=0.0,
                K=camera(rows, cols), gamma=GAMMA)


WIDE_BASE = 0x3FF5A5A5A5A5A5A5  # 1.35...: a mantissa of alternating bit pairs, so that flipping one bit moves up as often as down


def wide_ratios(rows, cols, salt=19):
    """ratios spanning 2^-40 .. 2^40 (and, through the exponent's bits, far beyond) around a base value that a third of the pixels carry exactly, another third with ONE bit of its
    pattern flipped (each of the 62 bits below the sign and the top exponent bit), the rest log-uniform over the whole span: the median is
    the base value wherever the frame is large enough, and in every radix pass patterns that share its prefix differ in the digit"""
    r = _rng(rows, cols, salt)
    base = np.array([WIDE_BASE], dtype=np.uint64)
    flips = base ^ (np.uint64(1) << np.arange(62, dtype=np.uint64))
    wide = np.exp2(np.linspace(-40.0, 40.0, 62))  # the ends exactly
    wide[1:-1] *= r.uniform(1.0, 1.5, size=60)
    vals = np.concatenate([np.repeat(base, 62).view(np.float64), flips.view(np.float64), wide])
    return planted_case(rows, cols, vals, 0.8, salt)


def two_values_on_the_boundary(rows, cols):
    """exactly two distinct ratios one unit in the last place apart, (n - 1) // 2 + 1 of the smaller: the rank (n - 1) // 2 is the LAST of the
    smaller value, and one correspondence that moved to the larger would make the median the larger"""
    d = planted_case(rows, cols, [1.25], share=1.0)
    n = rows * cols
    flat = d["Zn"].reshape(-1)
    flat[:] = 1.25
    perm = _rng(rows, cols, 23).permutation(n)
    flat[perm[: n - ((n - 1) // 2 + 1)]] = 1.25 * (1 + 2.0 ** -52)  # one unit in the last place above
    return d


# ---- the accuracy scene ---------------------------------------------------------------------------------------------------------------------------------
ACC_ROWS, ACC_COLS, ACC_SPEEDS = 96, 128, (1.0, 1.5, 1.0)
ACC_NOISE, ACC_OUTLIERS, ACC_SEED = 0.05, 0.10, 0x5EED0200
ACC_TRIALS, ACC_TOL, ACC_SOLVE_SEED = 50, 0.002, 7
# measured on the CPU (tests/test_link_cpu.py: test_scale_accuracy_through_the_oracle prints it): the larger of the two links' errors, and the
# bound the CPU and the GPU tests hold it to -- that error plus half of it, for the last-digit differences of the GPU solve
ACC_MEASURED = 0.030782
ACC_BOUND = 1.5 * ACC_MEASURED


def accuracy_scene(synth):
    """three pairs of the synthetic scene (synth.make_flow: model fields with 0.05 px noise and 10 % outliers, one realisation per pair) whose
    translations are 1, 1.5 and 1 times the default motion's.  -> dict(fields [3], K, gamma, v [3], w, k)"""
    rows, cols = ACC_ROWS, ACC_COLS
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = synth.default_motion()
    fields, vs = [], []
    for q, s in enumerate(ACC_SPEEDS):
        f, _ = synth.make_flow(rows, cols, K, s * v, w, k, GAMMA, ACC_NOISE, ACC_OUTLIERS, ACC_SEED + 16 * q)
        fields.append(f)
        vs.append(s * v)
    return dict(fields=fields, K=K, gamma=GAMMA, v=vs, w=w, k=k)


def speed_ratio_errors(scales, vs):
    """|(S_{q+1} |v_{q+1}|) / (S_q |v_q|) / (true speed ratio) - 1| for the two links: independent of how the solver normalises v"""
    est = [scales[q] * np.linalg.norm(vs[q]) for q in range(3)]
    return [abs((est[q + 1] / est[q]) / (ACC_SPEEDS[q + 1] / ACC_SPEEDS[q]) - 1.0) for q in range(2)]
