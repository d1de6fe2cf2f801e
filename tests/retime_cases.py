"""Inputs of the retimer's tests (tests/test_retime_cpu.py, tests/test_gpu_retime.py) and of its golden fixture
(tests/golden/make_golden_retime.py): layers for the merge alone at the shapes where its kernel can go wrong, the exact shift scene, frame
cases built from the occlusion test's scenes (tests/stabilize_visible_cases.py, reused as they are), seeded random tiny frames, and the
accuracy scene."""
import numpy as np

import link_spec_numpy as link
import retime_spec_numpy as spec
import stabilize_cases as stab_cases
import stabilize_visible_cases as vcases

# 2 x 2: one word; 3 x 7: a byte tail of 1; 5 x 5: tail 1, odd; 16 x 64: whole words; 37 x 67: tail 3, 3 workgroups; 16 x 131; 70 x 300: 21 workgroups
MERGE_SHAPES = [(2, 2), (3, 7), (5, 5), (16, 64), (37, 67), (16, 131), (70, 300)]
MERGE_WEIGHTS = [1, 32768, 32769, 65535]
MERGE_THRESHOLDS = [0, 24, 255]


def merge_layers(rows, cols, channels, seed=0):
    """two layers whose masks hold runs of all-zero words, all-set words, every mixed pattern and values other than 0 / 1, and whose images
    agree exactly, nearly (|d| <= 30) or not at all where both are set -- and hold random bytes where the mask is 0, which may not show.
    -> image_a, mask_a, image_b, mask_b"""
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed)
    n = rows * cols
    i = np.arange(n)

    def mask(phase):
        word = (i // 4 + phase) % 24  # words 0 .. 5 empty, 6 .. 11 set, 12 .. 23 every pattern of 4 bits but two
        bits = np.where(word < 6, 0, np.where(word < 12, 1, ((word - 11) >> (i % 4)) & 1))
        return (bits * rng.choice(np.array([1, 1, 2, 77, 128, 255]), size=n)).astype(np.uint8).reshape(rows, cols)

    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    image_a = rng.integers(0, 256, size=shape, dtype=np.uint8)
    kind = rng.integers(0, 3, size=(rows, cols))
    kind = kind if channels == 1 else kind[..., None]
    near = np.clip(image_a.astype(np.int64) + rng.integers(-30, 31, size=shape), 0, 255)
    image_b = np.where(kind == 0, image_a, np.where(kind == 1, near, rng.integers(0, 256, size=shape))).astype(np.uint8)
    return image_a, mask(0), image_b, mask(9)


def texture(rows, cols, channels, rng, noise=3):
    """a smooth texture with a little noise: two renders of it from slightly different poses agree within the default threshold nearly
    everywhere, and disagree at strong edges"""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    g = 128.0 + 60.0 * np.sin(x / 5.0 + rng.random() * 6.0) * np.cos(y / 4.0 + rng.random() * 6.0) + 30.0 * np.sin((x + y) / 7.0)
    g = g + rng.integers(-noise, noise + 1, size=(rows, cols))
    planes = g if channels == 1 else np.stack([g, 0.9 * g + 12.0, 1.1 * g - 12.0], axis=-1)
    return np.clip(np.rint(planes), 0, 255).astype(np.uint8)


def _frame_case(name, images, depths, Rs, ts, K, M, m, weight, window=None, threshold=spec.THRESHOLD_DEFAULT, occlusion=0, search=0, tol_q16=0, mode=0, q5_mode=0,
                iterations=0):
    rows, cols = depths[0].shape
    return dict(name=name, images=list(images), depths=list(depths), Rs=list(Rs), ts=list(ts), K=K, M=np.asarray(M, dtype=np.float64).reshape(-1, 3, 3),
                m=np.asarray(m, dtype=np.float64).reshape(-1, 3), weight=int(weight), window=tuple(window) if window else (0, 0, rows, cols), threshold=int(threshold),
                occlusion=int(occlusion), search=int(search), tol_q16=int(tol_q16), mode=mode, q5_mode=q5_mode, iterations=iterations)


SHIFT = 8  # columns between the shift scene's two frames; a multiple of 2, so that t = 0.5 moves each by whole pixels


def shift_case():
    """the stabiliser's shift scene seen by two cameras: constant depth 4, identity pose tables, K = (32, 32, 20, 12) at 24 x 40; frame 1 is
    frame 0's periodic integer texture (period 16 columns) SHIFT columns on, frame1[y, x] = frame0[y, x + SHIFT], which is what a camera moved
    by c1 - c0 = (SHIFT z / fx, 0, 0) = (1, 0, 0) sees.  At t = 0.5 layer a shows frame 0 moved by -SHIFT / 2 columns and layer b frame 1
    moved by +SHIFT / 2: the same bytes wherever both are set"""
    rows, cols = 24, 40
    base = np.random.default_rng(2440).integers(0, 256, size=(rows, 16, 3), dtype=np.uint8)
    frame = lambda off: base[:, (np.arange(cols) + off) % 16]
    depth = np.full((rows, cols), 4.0)
    R, t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
    K = (32.0, 32.0, 20.0, 12.0)
    A, c = np.stack([np.eye(3), np.eye(3)]), np.array([[0.0, 0.0, 0.0], [SHIFT * 4.0 / 32.0, 0.0, 0.0]])
    p = spec.retime_poses(A, c, A, c, np.ones(2), 2, 0.5)
    case = _frame_case("shift", [frame(0), frame(SHIFT)], [depth, depth], [R, R], [t, t], K, p["M"], p["m"], p["weight"])
    case.update(A=A, c=c, scales=np.ones(2))
    return case


def fold_pair(rows, cols, channels, occlusion=0, search=0, weight=20000, window=None, name=None, threshold=spec.THRESHOLD_DEFAULT):
    """the fold scene (a near box over a far background) from the left and from the right: two sources, two folds"""
    a, b = vcases.fold_case(rows, cols, channels, 1), vcases.fold_case(rows, cols, channels, -1)
    name = name or "fold-%dx%d-%s-occ%d%d" % (rows, cols, "bgr" if channels == 3 else "gray", occlusion, search)
    return _frame_case(name, [a["image"], b["image"]], [a["depth"], b["depth"]], [a["R"], b["R"]], [a["t"], b["t"]], a["K"], [a["M"], b["M"]], [a["m"], b["m"]], weight,
                       window, threshold, occlusion, search)


def smooth_pair(rows, cols, channels, seed, weight, threshold=spec.THRESHOLD_DEFAULT, occlusion=0, search=0, name=None, iterations=0):
    """a smooth texture over a smooth depth with a nearer box, two nearly equal frames seen from two nearby poses: mostly dissolved, conflicts at
    the box's edges, a-only and b-only bands at the frame's"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    depth = 6.0 + 2.0 * np.sin(x / 9.0 + rng.random()) * np.cos(y / 7.0 + rng.random())
    r0, c0 = int(rng.integers(0, rows)), int(rng.integers(0, cols))
    depth[r0:r0 + int(rng.integers(1, rows // 2 + 2)), c0:c0 + int(rng.integers(1, cols // 2 + 2))] = rng.uniform(1.5, 3.0)
    image = texture(rows, cols, channels, rng)
    image[r0:r0 + 2, c0:c0 + 3] = 255 - image[r0:r0 + 2, c0:c0 + 3]  # a strong edge
    other = np.clip(image.astype(np.int64) + rng.integers(-4, 5, size=image.shape), 0, 255).astype(np.uint8)
    R, t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
    K = (float(rng.uniform(20.0, 60.0)),) * 2 + (cols / 2.0 - 0.3, rows / 2.0 + 0.2)
    M = [link.rodrigues(rng.normal(size=3) * 0.01) for _ in range(2)]
    m = [rng.normal(size=3) * np.array([0.3, 0.3, 0.1]) for _ in range(2)]
    return _frame_case(name or "smooth-%dx%d-%d" % (rows, cols, seed), [image, other], [depth, depth.copy()], [R, R], [t, t], K, M, m, weight, None, threshold, occlusion,
                       search, iterations=iterations)


def random_case(seed):
    """a tiny frame pair drawn from `seed`: rows, cols in 2 .. 70, gray or BGR, any weight, one of four thresholds, each render call"""
    rng = np.random.default_rng(10007 * seed + 3)
    rows, cols = int(rng.integers(2, 71)), int(rng.integers(2, 71))
    occlusion = int(rng.integers(0, 2))
    return smooth_pair(rows, cols, 3 if rng.random() < 0.5 else 1, 500 + seed, int(rng.integers(1, 65536)), int(rng.choice([0, 8, 24, 255])), occlusion,
                       occlusion * int(rng.integers(0, 2)), name="random-%d" % seed, iterations=int(rng.integers(0, 4)))


def dense_pair(pose_table, name, rows, cols, channels, **kw):
    """the dense rectifier's inputs with its rolling-shutter pose table, the same frame seen from two poses"""
    a = vcases.dense_case(pose_table, name, rows, cols, channels=channels, **kw)
    return _frame_case(name, [a["image"]] * 2, [a["depth"]] * 2, [a["R"]] * 2, [a["t"]] * 2, a["K"], [vcases.M_N, stab_cases.M_STD], [vcases.m_N, stab_cases.m_STD], 40000)


def one_source(case, name):
    """a case's first source alone: an integer instant"""
    return dict(case, name=name, images=case["images"][:1], depths=case["depths"][:1], Rs=case["Rs"][:1], ts=case["ts"][:1], M=case["M"][:1], m=case["m"][:1], weight=0)


def all_cases(pose_table):
    """-> list of frame cases, names unique"""
    out = [shift_case()]
    out += [fold_pair(r, c, ch, occ, srch) for (r, c), ch, occ, srch in (((24, 40), 3, 0, 0), ((37, 67), 1, 1, 0), ((16, 131), 3, 1, 1), ((37, 67), 3, 0, 0))]
    h = 37 - 5
    out.append(fold_pair(37, 67, 3, 1, 1, weight=50000, window=(2, 3, h, (h * 67) // 37), name="fold-zoom", threshold=255))
    out.append(smooth_pair(37, 67, 3, 1, 32768))
    out.append(smooth_pair(16, 131, 1, 2, 32769, threshold=0))
    out.append(smooth_pair(33, 70, 3, 3, 1, occlusion=1))
    out.append(dense_pair(pose_table, "rs-table", 33, 70, 3, holes=0.0))
    out.append(dense_pair(pose_table, "holes", 33, 70, 1, holes=0.4))
    out.append(dense_pair(pose_table, "2x2", 2, 2, 3, holes=0.0))
    out.append(one_source(smooth_pair(37, 67, 3, 4, 0), "one-source"))
    out.append(one_source(dense_pair(pose_table, "x", 33, 70, 1, none_valid=True), "no-valid-depth"))
    assert len({c["name"] for c in out}) == len(out)
    return out


def run_spec(case):
    """the definition on a case.  -> dict(image, mask, source, counts, layers)"""
    return spec.retime_frame(case["images"], case["depths"], case["Rs"], case["ts"], case["K"], case["M"], case["m"], case["weight"], case["window"], case["threshold"],
                             case["occlusion"], case["search"], case["tol_q16"], case["mode"], case["q5_mode"], case["iterations"])


def accuracy_scene(synth, rows=96, cols=128, seed=0x5EED0000):
    """tests/test_stabilize_cpu.py's accuracy scene (the analytic texture on the TRUE smooth depth) as a static scene seen by global-shutter
    cameras: pose 0 the identity, pose 1 that test's (M, m), and the pose at t = 0.5 between them on the path.  A frame at a pose is the
    texture at the pre-image of every pixel under the true forward map, inverted by 50 fixed-point iterations; its depth map on its own grid
    is the true depth in that camera at the pre-image.  -> dict(frames [2], depths [2], R, t, K, A, c, scales, truth, inner, flow)"""
    import stabilize_spec_numpy as stab

    K = (0.8 * cols, 0.8 * cols, cols / 2.0 - 0.3, rows / 2.0 + 0.2)
    depth = synth.scene_depth(rows, cols)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    R, t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
    M1, m1 = stab_cases.M_STD, stab_cases.m_STD
    A = np.stack([np.eye(3), M1.T])  # X_1 = M X_0 + m  <=>  X_0 = A_1 X_1 + c_1
    c = np.stack([np.zeros(3), -(M1.T @ m1)])

    def view(M, m):
        gx, gy, _ = stab.forward_map(depth, R, t, *K, M, m)
        F = np.stack([gx - xx, gy - yy], axis=-1)
        px, py = xx.copy(), yy.copy()
        for _ in range(50):
            d = synth._bilinear(F, px, py)
            px, py = xx - d[..., 0], yy - d[..., 1]
        X = np.stack([depth * (xx - K[2]) / K[0], depth * (yy - K[3]) / K[1], depth], axis=-1)
        zv = X @ np.asarray(M)[2] + m[2]  # the depth in the moved camera, on camera 0's grid
        return synth._texture(px, py, seed), synth._bilinear(zv[..., None], px, py)[..., 0], F

    A_t, c_t = spec.path_at(A, c, 0.5)
    truth, _, _ = view(A_t.T, -(A_t.T @ c_t))
    f1, z1, F = view(M1, m1)
    frames = [np.rint(synth._texture(xx, yy, seed)).astype(np.uint8), np.rint(f1).astype(np.uint8)]
    band = int(np.ceil(np.abs(F).max())) + 3
    inner = np.zeros((rows, cols), dtype=bool)
    inner[band:rows - band, band:cols - band] = True
    return dict(frames=frames, depths=[depth, z1], R=R, t=t, K=K, A=A, c=c, scales=np.ones(2), truth=truth, inner=inner, flow=F)
