"""Inputs of the synthetic shutter's tests (tests/test_shutter_cpu.py, tests/test_gpu_shutter.py) and of its golden fixture
(tests/golden/make_golden_shutter.py): samples for the accumulate alone at the shapes where its kernel can go wrong, and small solved clips for
the frame call, built from the retimer's and the occlusion test's scenes (tests/retime_cases.py, tests/stabilize_visible_cases.py, reused as
they are)."""
import numpy as np

import link_spec_numpy as link
import retime_cases as rcases
import retime_spec_numpy as retime
import shutter_spec_numpy as spec
import stabilize_visible_cases as vcases

# the merge's shapes: one word; byte tails of 1 and 3; whole words; 3 workgroups; 21 workgroups
ACC_SHAPES = rcases.MERGE_SHAPES
ACC_SAMPLES = [1, 2, 3, 64]


def sample_mask(rows, cols, phase, rng):
    """retime_cases.merge_layers' pattern at a phase -- words (i // 4 + phase) % 24: 0 .. 5 empty, 6 .. 11 set, 12 .. 23 every pattern of 4 bits but
    two, set bytes drawn from values other than 0 / 1 too -- except that every seventh word is set in every sample and the word behind it empty
    in every sample, so that full and unset pixels exist whatever the number of samples"""
    n = rows * cols
    i = np.arange(n)
    word = (i // 4 + phase) % 24
    bits = np.where(word < 6, 0, np.where(word < 12, 1, ((word - 11) >> (i % 4)) & 1))
    bits = np.where((i // 4) % 7 == 0, 1, np.where((i // 4) % 7 == 1, 0, bits))
    return (bits * rng.choice(np.array([1, 1, 2, 77, 128, 255]), size=n)).astype(np.uint8).reshape(rows, cols)


def samples(rows, cols, channels, S, seed=0):
    """S samples (image, mask): random bytes everywhere -- also under empty mask bytes, where they may not show -- and the pattern above at a
    different phase per sample"""
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed + 17 * S)
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    return [(rng.integers(0, 256, size=shape, dtype=np.uint8), sample_mask(rows, cols, 5 * j + seed, rng)) for j in range(S)]


def saturated(rows, cols, channels, S=64):
    """S samples of 255, all set: the largest sums a cell can hold"""
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    return [(np.full(shape, 255, dtype=np.uint8), np.full((rows, cols), 255 if j % 2 else 1, dtype=np.uint8)) for j in range(S)]


def division_pairs():
    """every (s, n) with 1 <= n <= 64 and 0 <= s <= 255 n as the pixels of 64 gray samples: pixel i of sample j is set iff j < n_i and holds
    s_i // n_i + (j < s_i % n_i), so that its sum is s_i over n_i samples.  -> (samples [64] of (352, 1507) planes, s, n).  There are
    sum_n (255 n + 1) = 530 464 such pairs (256 * 2080 = 532 480 would count sums up to 256 n - 1, which no samples of bytes reach and whose
    mean, 256, is no byte)"""
    n = np.concatenate([np.full(255 * k + 1, k) for k in range(1, 65)])
    s = np.concatenate([np.arange(255 * k + 1) for k in range(1, 65)])
    assert n.size == 530464 == 352 * 1507
    out = []
    for j in range(64):
        out.append(((s // n + (j < s % n)).astype(np.uint8).reshape(352, 1507), (j < n).astype(np.uint8).reshape(352, 1507)))
    return out, s, n


# ---------------------------------------------------------------------------------------------------
# clips for the frame call
# ---------------------------------------------------------------------------------------------------
def _clip(name, frames, depths, Rs, ts, K, A, c, A_path, c_path, scales, t, shutter, samples, min_samples=1, window=None, threshold=retime.THRESHOLD_DEFAULT, occlusion=0,
          search=0, tol_q16=0, mode=0, q5_mode=0, iterations=0):
    rows, cols = depths[0].shape
    f64 = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))
    return dict(name=name, frames=list(frames), depths=list(depths), Rs=list(Rs), ts=list(ts), K=K, A=f64(A, (-1, 3, 3)), c=f64(c, (-1, 3)), A_path=f64(A_path, (-1, 3, 3)),
                c_path=f64(c_path, (-1, 3)), scales=f64(scales, (-1,)), t=float(t), shutter=float(shutter), samples=int(samples), min_samples=int(min_samples),
                window=tuple(window) if window else (0, 0, rows, cols), threshold=int(threshold), occlusion=int(occlusion), search=int(search), tol_q16=int(tol_q16),
                mode=mode, q5_mode=q5_mode, iterations=iterations)


def shift_clip(t=0.5625, shutter=0.5, samples=4, min_samples=1, name="shift"):
    """retime_cases.shift_case as a clip of two sources riding its own chain: the sub-instant t_j shows the periodic texture moved by exactly
    8 t_j columns wherever 8 t_j is an integer.  The defaults give the sub-instants 0.375, 0.5, 0.625, 0.75: moved by 3, 4, 5, 6 columns"""
    s = rcases.shift_case()
    return _clip(name, s["images"], s["depths"], s["Rs"], s["ts"], s["K"], s["A"], s["c"], s["A"], s["c"], s["scales"], t, shutter, samples, min_samples)


def shift_base():
    """the shift scene's texture over one period: (24, 16, 3); frame 0 is base[:, x % 16]"""
    return rcases.shift_case()["images"][0][:, :16]


def fold_clip(rows, cols, channels, occlusion=0, search=0, t=0.5, shutter=0.5, samples=3, min_samples=1, window=None, name=None, threshold=retime.THRESHOLD_DEFAULT):
    """the fold scene from the left and from the right as a clip of two sources: at t = 0.5 the camera stands where retime_cases.fold_pair's
    does, and the path rides a third of the way from one source to the other"""
    a, b = vcases.fold_case(rows, cols, channels, 1), vcases.fold_case(rows, cols, channels, -1)
    A = [np.eye(3), np.eye(3)]
    c = [[-vcases.SHIFT, 0.0, 0.0], [vcases.SHIFT, 0.0, 0.0]]
    A_path = [link.rodrigues(np.array([0.0, -0.004, 0.0])), link.rodrigues(np.array([0.002, 0.004, -0.003]))]
    c_path = [[-vcases.SHIFT / 3, 0.0, 0.0], [vcases.SHIFT / 3, 0.01, 0.0]]
    name = name or "fold-%dx%d-%s-occ%d%d" % (rows, cols, "bgr" if channels == 3 else "gray", occlusion, search)
    return _clip(name, [a["image"], b["image"]], [a["depth"], b["depth"]], [a["R"], b["R"]], [a["t"], b["t"]], a["K"], A, c, A_path, c_path, np.ones(2), t, shutter, samples,
                 min_samples, window, threshold, occlusion, search)


def smooth_clip(rows, cols, channels, seed, t, shutter, samples, min_samples=1, nsources=3, name=None, **kw):
    """retime_cases.smooth_pair's scene as a clip of nsources frames that differ by a little noise, the chain a steady walk with a steady turn
    and the path a slower one beside it, so that an integer instant is no source's own pose; scales other than 1"""
    p = rcases.smooth_pair(rows, cols, channels, seed, 1)
    rng = np.random.default_rng(seed + 77)
    frames = list(p["images"])
    while len(frames) < nsources:
        frames.append(np.clip(frames[0].astype(np.int64) + rng.integers(-4, 5, size=frames[0].shape), 0, 255).astype(np.uint8))
    w, step = np.array([0.004, -0.006, 0.003]), np.array([0.9, 0.4, 0.1])
    A = [link.rodrigues(n * w) for n in range(nsources)]
    c = [n * step for n in range(nsources)]
    A_path = [link.rodrigues(0.8 * n * w) for n in range(nsources)]
    c_path = [0.5 * n * step + np.array([0.4, -0.3, -0.05]) for n in range(nsources)]
    scales = 1.0 + 0.05 * np.arange(nsources)
    return _clip(name or "smooth-%dx%d-%d" % (rows, cols, seed), frames[:nsources], [p["depths"][0]] * nsources, [p["Rs"][0]] * nsources, [p["ts"][0]] * nsources, p["K"], A, c,
                 A_path, c_path, scales, t, shutter, samples, min_samples, **kw)


def dense_clip(pose_table, name, rows, cols, channels, t=0.5, shutter=0.5, samples=2, **kw):
    """the dense rectifier's inputs with its rolling-shutter pose table as a clip of two equal frames seen from two poses"""
    a = vcases.dense_case(pose_table, name, rows, cols, channels=channels, **kw)
    A = [np.eye(3), link.rodrigues(np.array([0.01, -0.02, 0.005]))]
    c = [[0.0, 0.0, 0.0], [0.05, -0.02, 0.01]]
    return _clip(name, [a["image"]] * 2, [a["depth"]] * 2, [a["R"]] * 2, [a["t"]] * 2, a["K"], A, c, A, c, np.ones(2), t, shutter, samples)


def all_cases(pose_table):
    """-> list of frame cases, names unique: the shift scene; a fold pair through the occlusion test and through the search; a smooth clip of
    three sources whose window spans an integer instant; a zoomed window; the 2 x 2 dense case; a window clipped at t = 0; an integer t; the two
    identity forms (shutter = 0, S = 1); min_samples = S"""
    h = 37 - 5
    out = [shift_clip(),
           fold_clip(24, 40, 3, 1, 0),
           fold_clip(37, 67, 1, 1, 1, t=0.4, shutter=0.6, samples=4),
           smooth_clip(37, 67, 3, 1, t=1.0, shutter=1.0, samples=5),
           smooth_clip(16, 131, 1, 2, t=1.3, shutter=0.7, samples=4, min_samples=4, name="smooth-all-four"),
           fold_clip(37, 67, 3, 0, 0, window=(2, 3, h, (h * 67) // 37), name="fold-zoom", threshold=255),
           dense_clip(pose_table, "2x2", 2, 2, 3, holes=0.0),
           smooth_clip(33, 70, 3, 3, t=0.1, shutter=0.5, samples=4, name="clipped-at-0"),
           smooth_clip(33, 70, 1, 4, t=2.0, shutter=0.5, samples=3, min_samples=3, name="clipped-at-the-end"),
           smooth_clip(33, 70, 3, 5, t=1.0, shutter=0.5, samples=3, name="integer-t"),
           smooth_clip(33, 70, 3, 6, t=0.7, shutter=0.0, samples=5, name="shutter-0"),
           smooth_clip(33, 70, 1, 7, t=0.7, shutter=0.9, samples=1, name="one-sample")]
    assert len({c["name"] for c in out}) == len(out)
    return out


def run_spec(case):
    """the definition on a case.  -> dict(image, mask, coverage, counts, times, samples)"""
    return spec.shutter_frame(case["frames"], case["depths"], case["Rs"], case["ts"], case["K"], case["A"], case["c"], case["A_path"], case["c_path"], case["scales"],
                              case["t"], case["shutter"], case["samples"], case["min_samples"], case["window"], case["threshold"], case["occlusion"], case["search"],
                              case["tol_q16"], case["mode"], case["q5_mode"], case["iterations"])


def retimed(case):
    """the retimed frame at the case's t itself (tests/retime_spec_numpy.py): what shutter = 0 and S = 1 must give"""
    n = len(case["depths"])
    p = retime.retime_poses(case["A"], case["c"], case["A_path"], case["c_path"], case["scales"], n, case["t"])
    src = p["sources"]
    return retime.retime_frame([case["frames"][q] for q in src], [case["depths"][q] for q in src], [case["Rs"][q] for q in src], [case["ts"][q] for q in src], case["K"],
                               p["M"], p["m"], p["weight"], case["window"], case["threshold"], case["occlusion"], case["search"], case["tol_q16"], case["mode"],
                               case["q5_mode"], case["iterations"])
