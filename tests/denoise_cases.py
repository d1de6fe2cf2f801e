"""Inputs of the temporal denoise's tests (tests/test_denoise_cpu.py, tests/test_gpu_denoise.py) and of its golden fixture
(tests/golden/make_golden_denoise.py): references and layers for the accumulate alone at the shapes where its kernel can go wrong (a tile is
16 rows x 64 columns), records that drive every gain clamp, the impulse positions, and small solved clips for the frame and clip calls, built
from the retimer's, the shutter's and the occlusion test's scenes (tests/retime_cases.py, tests/shutter_cases.py, reused as they are)."""
import numpy as np

import denoise_spec_numpy as spec
import retime_cases as rcases
import retime_spec_numpy as retime
import shutter_cases as scases
import stabilize_fill_spec_numpy as fill

TILE_ROWS, TILE_COLS = 16, 64
# one word; odd sizes with byte tails; one under, exactly one and one over the tile in both directions; several tiles with rows that start on
# every byte of a dword (cols % 4 = 3, 3, 1, 0)
ACC_SHAPES = [(2, 2), (3, 7), (5, 5), (15, 63), (16, 64), (17, 65), (16, 131), (37, 67), (33, 129), (70, 300)]
ACC_LAYERS = [1, 2, 14]

# records [count, sum image_c, sum layer_c, 0 ...] by channels: the gain clamped from below (16384), from above (262144), a plain gain of 1.1 and
# 0.9 per channel, too small an overlap (no gain), and a layer sum of 0 (no gain)
def records(ch):
    def rec(count, si, sl):
        out = np.zeros(8, dtype=np.uint64)
        out[0] = count
        out[1:1 + ch] = si[:ch]
        out[1 + ch:1 + 2 * ch] = sl[:ch]
        return out

    return dict(low=rec(5000, [100, 200, 150], [1000, 1000, 1000]), high=rec(5000, [5000, 9000, 262144], [1000, 1000, 1]),
                plain=rec(5000, [1100, 900, 1000], [1000, 1000, 1001]), small=rec(1023, [2000, 2000, 2000], [1000, 1000, 1000]),
                zero=rec(5000, [1000, 1000, 1000], [0, 1000, 0]))


def reference(rows, cols, channels, seed=0):
    """(image, mask): random bytes everywhere -- also under empty mask bytes -- and shutter_cases.sample_mask's pattern (empty words, full words,
    every mixed pattern, values other than 0 / 1)"""
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed + 5)
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    return rng.integers(0, 256, size=shape, dtype=np.uint8), scases.sample_mask(rows, cols, 3 + seed, rng)


def layers(ref, rows, cols, channels, L, seed=0):
    """L layers (image, mask): per pixel the reference's bytes, the reference within +-3, within +-20, or random bytes, in patches of 3 x 5 so that
    the patch errors -- and the weights -- take every value from 0 to 16; masks at a different phase per layer; random bytes under empty mask bytes"""
    rng = np.random.default_rng(rows * 7919 + cols * 31 + channels + 1000 * seed + 17 * L + 9)
    out = []
    r = ref.astype(np.int64)
    for j in range(L):
        kind = rng.integers(0, 4, size=((rows + 2) // 3, (cols + 4) // 5)).repeat(3, axis=0).repeat(5, axis=1)[:rows, :cols]
        kind = kind if channels == 1 else kind[..., None]
        near = np.clip(r + rng.integers(-3, 4, size=r.shape), 0, 255)
        far = np.clip(r + rng.integers(-20, 21, size=r.shape), 0, 255)
        img = np.where(kind == 0, r, np.where(kind == 1, near, np.where(kind == 2, far, rng.integers(0, 256, size=r.shape)))).astype(np.uint8)
        out.append((img, scases.sample_mask(rows, cols, 5 * j + seed + 1, rng)))
    return out


def impulse_positions(rows, cols):
    """every corner and every edge midpoint of a tile and of the frame, inside the frame, unique"""
    ys = {0, rows - 1, rows // 2}
    xs = {0, cols - 1, cols // 2}
    for y0 in range(0, rows, TILE_ROWS):
        ys |= {y0, min(y0 + TILE_ROWS - 1, rows - 1), min(y0 + TILE_ROWS // 2, rows - 1)}
    for x0 in range(0, cols, TILE_COLS):
        xs |= {x0, min(x0 + TILE_COLS - 1, cols - 1), min(x0 + TILE_COLS // 2, cols - 1)}
    return sorted((y, x) for y in ys for x in xs)


# ---------------------------------------------------------------------------------------------------
# clips for the frame and the clip call
# ---------------------------------------------------------------------------------------------------
def _clip(name, frames, depths, Rs, ts, K, A, c, A_path, c_path, scales, q, radius=spec.RADIUS_DEFAULT, strength=spec.STRENGTH_DEFAULT, window=None,
          min_overlap=spec.MIN_OVERLAP_DEFAULT, gain_mode=0, occlusion=0, search=0, tol_q16=0, mode=0, q5_mode=0, iterations=0):
    rows, cols = depths[0].shape
    f64 = lambda a, shape: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))
    return dict(name=name, frames=list(frames), depths=list(depths), Rs=list(Rs), ts=list(ts), K=K, A=f64(A, (-1, 3, 3)), c=f64(c, (-1, 3)), A_path=f64(A_path, (-1, 3, 3)),
                c_path=f64(c_path, (-1, 3)), scales=f64(scales, (-1,)), q=int(q), radius=int(radius), strength=int(strength),
                window=tuple(window) if window else (0, 0, rows, cols), min_overlap=int(min_overlap), gain_mode=int(gain_mode), occlusion=int(occlusion), search=int(search),
                tol_q16=int(tol_q16), mode=mode, q5_mode=q5_mode, iterations=iterations)


def from_shutter(clip, name, q, **kw):
    """a shutter clip's sources, chain and path"""
    return _clip(name, clip["frames"], clip["depths"], clip["Rs"], clip["ts"], clip["K"], clip["A"], clip["c"], clip["A_path"], clip["c_path"], clip["scales"], q, **kw)


SHIFT_FRAMES = 5


def shift_clean(nframes=SHIFT_FRAMES, cols=40):
    """retime_cases.shift_case widened to five (or nframes) frames, its texture drawn from 32 .. 223 so that noise of +-6 never clips: frame n is the
    periodic texture (period 16 columns) moved on by SHIFT = 8 columns per frame, the camera by (1, 0, 0).  -> (clean frames, clip fields)"""
    s = rcases.shift_case()
    rows = s["depths"][0].shape[0]
    base = np.random.default_rng(2441).integers(32, 224, size=(rows, 16, 3), dtype=np.uint8)
    frames = [base[:, (np.arange(cols) + rcases.SHIFT * n) % 16] for n in range(nframes)]
    depth = np.full((rows, cols), 4.0)
    R, t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
    A = np.stack([np.eye(3)] * nframes)
    c = np.array([[n * rcases.SHIFT * 4.0 / 32.0, 0.0, 0.0] for n in range(nframes)])
    return frames, dict(depths=[depth] * nframes, Rs=[R] * nframes, ts=[t] * nframes, K=s["K"], A=A, c=c, scales=np.ones(nframes))


def shift_clip(seed=0, channels=3, q=2, radius=2, strength=spec.STRENGTH_DEFAULT, noise=6, name=None, nframes=SHIFT_FRAMES, cols=40):
    """the shift frames (five of 40 columns unless asked otherwise) with i.i.d. integer noise in [-noise, noise] per frame; the path is the
    chain itself.  The clean frames ride along as case["clean"]"""
    clean, f = shift_clean(nframes, cols)
    rng = np.random.default_rng(7000 + seed)
    if channels == 1:
        clean = [np.ascontiguousarray(fr[..., 1]) for fr in clean]
    frames = [(fr.astype(np.int64) + rng.integers(-noise, noise + 1, size=fr.shape)).astype(np.uint8) for fr in clean]
    case = _clip(name or "shift-%s-%d" % ("bgr" if channels == 3 else "gray", seed), frames, f["depths"], f["Rs"], f["ts"], f["K"], f["A"], f["c"], f["A"], f["c"], f["scales"],
                 q, radius, strength)
    case["clean"] = clean
    return case


def shift_seen_by_all(case):
    """the columns of frame q's camera that every source of the shift clip sees"""
    cols = case["depths"][0].shape[1]
    ok = np.ones(cols, dtype=bool)
    for n in spec.neighbour_order(case["q"], len(case["depths"]), case["radius"]):
        d = rcases.SHIFT * (n - case["q"])  # frame n's column x shows at column x + d
        seen = np.zeros(cols, dtype=bool)
        seen[max(d, 0):min(cols + d, cols)] = True
        ok &= seen
    return ok


def gained_clip():
    """a smooth clip of three sources whose neighbours are brighter and darker than the own frame: the record gives a gain other than 1"""
    clip = scases.smooth_clip(37, 67, 3, 11, t=1.0, shutter=0.0, samples=1, nsources=3)
    fr = clip["frames"]
    clip = dict(clip, frames=[np.clip(fr[0].astype(np.int64) * 5 // 4, 0, 255).astype(np.uint8), fr[1], np.clip(fr[2].astype(np.int64) * 4 // 5, 0, 255).astype(np.uint8)])
    return from_shutter(clip, "gained", 1, radius=1, strength=20)


def all_cases(pose_table):
    """-> list of frame cases, names unique: the noisy shift scene, gray and BGR; a fold pair plain, through the occlusion test and through the
    search; a zoomed window; the gained neighbours with the gain on and off; a smooth clip of five sources at radius 2 from its middle and, one
    sided, from its first frame; one source alone; the 2 x 2 dense case"""
    h = 37 - 5
    five = scases.smooth_clip(33, 70, 1, 21, t=1.0, shutter=0.0, samples=1, nsources=5)
    out = [shift_clip(0, 3), shift_clip(1, 1),
           from_shutter(scases.fold_clip(24, 40, 3), "fold-plain", 0, radius=1),
           from_shutter(scases.fold_clip(37, 67, 1, 1, 0), "fold-visible", 1, radius=1, occlusion=1),
           from_shutter(scases.fold_clip(37, 67, 3, 1, 1), "fold-search", 0, radius=1, occlusion=1, search=1, strength=40),
           from_shutter(scases.fold_clip(37, 67, 3), "fold-zoom", 0, radius=1, window=(2, 3, h, (h * 67) // 37), strength=255),
           gained_clip(), dict(gained_clip(), name="gain-off", gain_mode=1), dict(gained_clip(), name="gain-small-overlap", min_overlap=100000),
           from_shutter(five, "five-middle", 2, radius=2), from_shutter(five, "five-first", 0, radius=2, strength=1), from_shutter(five, "five-radius-7", 4, radius=7),
           from_shutter(scases.smooth_clip(16, 131, 3, 22, t=0.0, shutter=0.0, samples=1, nsources=1), "one-source", 0),
           from_shutter(scases.dense_clip(pose_table, "2x2", 2, 2, 3, holes=0.0), "2x2", 1, radius=1)]
    assert len({c["name"] for c in out}) == len(out)
    return out


def sources_and_poses(case, q=None):
    """frame q's sources (q first, then the fill's neighbour order) and their poses on the case's path -> (sources, M (nsrc, 3, 3), m (nsrc, 3))"""
    q = case["q"] if q is None else q
    ns = len(case["depths"])
    src = spec.neighbour_order(q, ns, case["radius"])
    own = retime.retime_poses(case["A"], case["c"], case["A_path"], case["c_path"], case["scales"], ns, float(q))
    M, m = [own["M"][0]], [own["m"][0]]
    for n in src[1:]:
        Mn, mn = fill.neighbour_pose(case["A"], case["c"], case["A_path"], case["c_path"], case["scales"], q, n)
        M.append(Mn)
        m.append(mn)
    return src, np.array(M), np.array(m)


def run_spec(case, q=None):
    """the definition on frame q of a case.  -> denoise_frame's dict plus sources"""
    src, M, m = sources_and_poses(case, q)
    pick = lambda k: [case[k][n] for n in src]
    r = spec.denoise_frame(pick("frames"), pick("depths"), pick("Rs"), pick("ts"), case["K"], M, m, case["window"], case["strength"], case["min_overlap"], case["gain_mode"],
                           case["occlusion"], case["search"], case["tol_q16"], case["mode"], case["q5_mode"], case["iterations"])
    return dict(r, sources=src)
