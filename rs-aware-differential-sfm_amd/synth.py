"""Analytic synthetic rolling-shutter flow generator (SURVEY.md section 8 d).

Produces model-consistent dense optical flow for a known scene depth Z(x, y), motion (v, w, k) and
readout ratio gamma, plus optional DeepFlow-like noise / outliers.  This replaces the reference's
MATLAB renderer (matlab_synthetic_data/*.m), which needs a closed-source MEX and mesh.

Data tooling for tests and bench (numpy, host side) -- not part of the solve.
"""
import numpy as np

# intrinsics (f_x, f_y, c_x, c_y).  galaxy / galaxy_vga are the reference's (camera.cc:189-200).
INTRINSICS = {
    "galaxy_vga": (484.450845764569, 485.345469134313, 313.442094604855, 241.383116350144),
    "galaxy": (1492.41306997746, 1491.09286590722, 949.571146410704, 554.675409391795),
    "hd720": (995.0, 994.0, 633.0, 370.0),
    "uhd": (2984.82613995492, 2982.18573181444, 1899.142292821408, 1109.35081878359),
}

# BASELINE.json configs -> (rows, cols, intrinsics, gamma, noise_px, outlier_frac)
CONFIGS = {
    1: dict(rows=480, cols=640, K="galaxy_vga", gamma=0.8, noise_px=0.0, outliers=0.0),
    2: dict(rows=720, cols=1280, K="hd720", gamma=0.8, noise_px=0.0, outliers=0.0),
    3: dict(rows=1080, cols=1920, K="galaxy", gamma=0.95, noise_px=0.3, outliers=0.10),
    4: dict(rows=2160, cols=3840, K="uhd", gamma=0.95, noise_px=0.3, outliers=0.10),
    5: dict(rows=720, cols=1280, K="hd720", gamma=0.8, noise_px=0.3, outliers=0.10),
}

_GAMMA64 = np.uint64(0x9E3779B97F4A7C15)


def splitmix64(seed, n):
    """n 64-bit outputs of splitmix64 started at `seed` (vectorised, identical to the scalar generator)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + _GAMMA64 * np.arange(1, n + 1, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniform01(seed, n):
    return (splitmix64(seed, n) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def normal(seed, n):
    u = uniform01(seed, 2 * n)
    u1 = np.maximum(u[:n], 1e-300)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u[n:])


def scene_depth(rows, cols):
    """Z(x, y) = 1 + 0.35 sin(2 pi 1.3 x/cols) cos(2 pi 0.9 y/rows) + 0.25 x/cols  (mean depth ~ 1)."""
    x = np.arange(cols, dtype=np.float64)[None, :]
    y = np.arange(rows, dtype=np.float64)[:, None]
    return 1.0 + 0.35 * np.sin(2 * np.pi * 1.3 * x / cols) * np.cos(2 * np.pi * 0.9 * y / rows) + 0.25 * (x / cols)


def make_flow(rows, cols, K, v, w, k=0.0, gamma=0.8, noise_px=0.0, outliers=0.0, seed=0x5EED0000, depth=None, _model_only=False):
    """Dense model-consistent RS flow image (rows, cols, 2) in pixels, row-major, plus ground truth.

    Model (minimal.cc:257-266):  u = beta (A v rho + B w),  u = flow_px * gamma / f,
    alpha = 1 + gamma flow_y/h, alpha_k = 0.5[(1 + gamma (y + flow_y)/h)^2 - (gamma y/h)^2], h = rows,
    beta = 2 (alpha + k alpha_k) / (2 + k).  alpha depends on the flow itself -> fixed point.
    """
    fx, fy, cx, cy = K
    v = np.asarray(v, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    Z = scene_depth(rows, cols) if depth is None else np.asarray(depth, dtype=np.float64)
    rho = 1.0 / Z
    xi = np.arange(cols, dtype=np.float64)[None, :]
    yj = np.arange(rows, dtype=np.float64)[:, None]
    x = (xi - cx) / fx + 0.0 * yj
    y = (yj - cy) / fy + 0.0 * xi
    m0 = (v[0] - x * v[2]) * rho + (-x * y) * w[0] + (1 + x * x) * w[1] + (-y) * w[2]
    m1 = (v[1] - y * v[2]) * rho + (-(1 + y * y)) * w[0] + (x * y) * w[1] + x * w[2]
    h = float(rows)
    fyy = np.zeros((rows, cols))
    for _ in range(60):
        alpha = 1.0 + gamma * fyy / h
        part1 = gamma * yj / h
        part2 = 1.0 + gamma * (yj + fyy) / h
        alpha_k = 0.5 * (part2 * part2 - part1 * part1)
        beta = 2.0 * (alpha + k * alpha_k) / (2.0 + k)
        new = beta * m1 * fy / gamma
        if np.max(np.abs(new - fyy)) < 1e-15:
            fyy = new
            break
        fyy = new
    alpha = 1.0 + gamma * fyy / h
    part1 = gamma * yj / h
    part2 = 1.0 + gamma * (yj + fyy) / h
    alpha_k = 0.5 * (part2 * part2 - part1 * part1)
    beta = 2.0 * (alpha + k * alpha_k) / (2.0 + k)
    fxx = beta * m0 * fx / gamma
    flow = np.stack([fxx, fyy], axis=-1)
    truth = dict(v=v, w=w, k=float(k), gamma=float(gamma), Z=Z, K=K)
    if _model_only:
        return np.ascontiguousarray(flow), truth
    flow, outlier_mask = add_noise(flow, noise_px, outliers, seed)
    truth["outlier_mask"] = outlier_mask
    return np.ascontiguousarray(flow), truth


def add_noise(flow, noise_px, outliers, seed):
    """DeepFlow-like degradation of a model flow field: Gaussian noise (pixels) and a fraction of uniform +-30 px outliers, both from
    splitmix64(seed) -- the second half of make_flow, callable on its own so that a SEQUENCE of pairs (one noise seed each) shares
    the model field.  Returns (flow, outlier mask)."""
    rows, cols = flow.shape[:2]
    n = rows * cols
    if noise_px > 0.0:
        flow = flow + noise_px * normal(seed + 1, 2 * n).reshape(rows, cols, 2)
    outlier_mask = np.zeros((rows, cols), dtype=bool)
    if outliers > 0.0:
        outlier_mask = uniform01(seed + 2, n).reshape(rows, cols) < outliers
        rnd = (uniform01(seed + 3, 2 * n).reshape(rows, cols, 2) * 2.0 - 1.0) * 30.0
        flow = np.where(outlier_mask[..., None], rnd, flow)
    return flow, outlier_mask


def make_flow_sequence(cfg, seeds):
    """flow images (rows, cols, 2) of BASELINE config `cfg` for several data seeds: the same scene and motion, one noise / outlier
    realisation per seed (each identical to make_config(cfg, seed=s)["flow_img"]); the model field is computed once"""
    c = CONFIGS[cfg]
    v, w, k = default_motion()
    K = INTRINSICS[c["K"]]
    base, truth = make_flow(c["rows"], c["cols"], K, v, w, k, c["gamma"], _model_only=True)
    imgs = [np.ascontiguousarray(add_noise(base, c["noise_px"], c["outliers"], s_)[0]) for s_ in seeds]
    return imgs, dict(rows=c["rows"], cols=c["cols"], K=K, gamma=c["gamma"], truth=truth)


def flatten_numpy(flow_img, K, gamma, thr=1e-10):
    """Host restatement of the caller glue main.cc:398-444 (column-major scan, shrinking variant
    errorMeasure.cpp:96-97) + getAlpha/getAlphaK (minimal.cc:179-197), for building solver inputs.
    Returns q, u (normalised, n x 2), alpha, alpha_k (n), and the column-major pixel index of each point."""
    fx, fy, cx, cy = K
    rows, cols = flow_img.shape[:2]
    f = np.transpose(flow_img, (1, 0, 2)).reshape(-1, 2)  # column-major scan: i over cols outer, j inner
    ii = np.repeat(np.arange(cols, dtype=np.float64), rows)
    jj = np.tile(np.arange(rows, dtype=np.float64), cols)
    keep = (f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) > thr
    f, ii, jj = f[keep], ii[keep], jj[keep]
    q = np.stack([(ii - cx) * 1.0 / fx, (jj - cy) * 1.0 / fy], axis=1)
    u = np.stack([f[:, 0] * gamma / fx, f[:, 1] * gamma / fy], axis=1)
    h = float(rows)
    alpha = 1 + gamma * f[:, 1] / h
    part1 = gamma * jj / h
    part2 = 1.0 + gamma * (jj + f[:, 1]) / h
    alpha_k = 0.5 * (part2 * part2 - part1 * part1)
    pix = np.nonzero(keep)[0]
    return (np.ascontiguousarray(q), np.ascontiguousarray(u), np.ascontiguousarray(alpha),
            np.ascontiguousarray(alpha_k), pix)


def _texture(x, y, seed):
    """procedural BGR texture at real coordinates: six octaves of seeded sinusoids (periods 256 .. 8 px, four directions each) --
    gradients at every pyramid scale -- plus a per-channel offset; float64 (rows, cols, 3) in [0, 255]"""
    u = uniform01(seed, 6 * 4 * 2)
    t = np.zeros(np.broadcast(x, y).shape)
    for o in range(6):
        freq = 2.0 * np.pi / (256.0 / 2 ** o)
        for j in range(4):
            th, ph = np.pi * u[8 * o + 2 * j], 2.0 * np.pi * u[8 * o + 2 * j + 1]
            t = t + (22.0 / (1.0 + 0.5 * o)) * np.sin(freq * (np.cos(th) * x + np.sin(th) * y) + ph)
    t = 128.0 + 0.55 * t
    return np.clip(np.stack([t, 0.9 * t + 12.0, 1.1 * t - 12.0], axis=-1), 0.0, 255.0)


def _bilinear(f, x, y):
    """f (rows, cols, ...) sampled at real (x, y), replicate border"""
    rows, cols = f.shape[:2]
    x = np.clip(x, 0.0, cols - 1.0)
    y = np.clip(y, 0.0, rows - 1.0)
    x0 = np.minimum(np.floor(x).astype(np.int64), cols - 2)
    y0 = np.minimum(np.floor(y).astype(np.int64), rows - 2)
    ax, ay = (x - x0)[..., None], (y - y0)[..., None]
    return ((1 - ay) * ((1 - ax) * f[y0, x0] + ax * f[y0, x0 + 1]) + ay * ((1 - ax) * f[y0 + 1, x0] + ax * f[y0 + 1, x0 + 1]))


def render_pair(rows, cols, K, v, w, k=0.0, gamma=0.8, seed=0x5EED0000):
    """Two 8-bit BGR frames of a procedural texture moved by make_flow's model flow F, for testing a flow estimator (the DeepFlow
    front end): frame 1 is the texture T, frame 2 at pixel q shows T(p) with p + F(p) = q (solved by p <- q - F(p), F bilinear).
    Returns (img1, img2, flow F (rows, cols, 2), valid mask): the mask leaves out a border band of max|F| + 5 pixels, where frame 2
    shows texture that frame 1 does not."""
    flow, _ = make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    img1 = np.rint(_texture(xx, yy, seed)).astype(np.uint8)
    px, py = xx.copy(), yy.copy()
    for _ in range(50):
        F = _bilinear(flow, px, py)
        nx, ny = xx - F[..., 0], yy - F[..., 1]
        done = max(np.abs(nx - px).max(), np.abs(ny - py).max()) < 1e-9
        px, py = nx, ny
        if done:
            break
    img2 = np.rint(_texture(px, py, seed)).astype(np.uint8)
    band = int(np.ceil(np.abs(flow).max())) + 5
    mask = np.zeros((rows, cols), dtype=bool)
    mask[band:rows - band, band:cols - band] = True
    return img1, img2, np.ascontiguousarray(flow), mask


def render_occluded_pair(rows, cols, K, v, w, k=0.0, gamma=0.8, seed=0x5EED0000, block=None, block_motion=(6, 0)):
    """render_pair's two frames with a textured rectangle pasted over both, moved by its own integer translation between them: a pair
    with a real occlusion, for testing the forward-backward flow check.  block = (y0, x0, h, w) is the rectangle in frame 1 (None: a
    quarter of each side, starting at a third), block_motion = (dx, dy) its translation; it must lie inside both frames.  Its texture is
    _texture in the block's own coordinates under another seed.  Returns (img1, img2, occluded, block_plane): occluded marks the
    frame-1 BACKGROUND pixels p whose landing point p + F(p) (F = render_pair's model flow), rounded to the nearest pixel, the block
    covers in frame 2 -- no flow can match them; block_plane marks the block's pixels in frame 1."""
    img1, img2, flow, _ = render_pair(rows, cols, K, v, w, k, gamma, seed)
    y0, x0, h, bw = (rows // 3, cols // 3, rows // 4, cols // 4) if block is None else (int(b) for b in block)
    dx, dy = (int(m) for m in block_motion)
    if min(y0, x0, y0 + dy, x0 + dx) < 0 or h < 1 or bw < 1 or max(y0, y0 + dy) + h > rows or max(x0, x0 + dx) + bw > cols:
        raise ValueError("the block must lie inside both frames")
    by, bx = np.mgrid[0:h, 0:bw].astype(np.float64)
    tex = np.rint(_texture(3.0 * bx, 3.0 * by, (seed ^ 0xB10C) & 0xFFFFFFFF)[..., ::-1]).astype(np.uint8)
    img1, img2 = img1.copy(), img2.copy()
    img1[y0:y0 + h, x0:x0 + bw] = tex
    img2[y0 + dy:y0 + dy + h, x0 + dx:x0 + dx + bw] = tex
    block_plane = np.zeros((rows, cols), dtype=bool)
    block_plane[y0:y0 + h, x0:x0 + bw] = True
    yy, xx = np.mgrid[0:rows, 0:cols]
    lx, ly = np.rint(xx + flow[..., 0]), np.rint(yy + flow[..., 1])
    covered = (lx >= x0 + dx) & (lx < x0 + dx + bw) & (ly >= y0 + dy) & (ly < y0 + dy + h)
    return img1, img2, covered & ~block_plane, block_plane


def _exposed(texture, gain):
    """one frame's bytes: the texture rounded, or with an exposure factor clip(rint(gain texture))"""
    if gain is None:
        return np.rint(texture).astype(np.uint8)
    return np.clip(np.rint(float(gain) * texture), 0, 255).astype(np.uint8)


def _sensor_noise(frames, noise, noise_seed):
    """seeded integer sensor noise on a stack of frames: every byte + an integer drawn uniformly from [-noise, noise], clipped to 0 .. 255, frame
    j from the generator seeded (noise_seed, j) -- so a frame's noise does not depend on how many frames follow it.  None or 0: the frames
    themselves"""
    if isinstance(noise, (tuple, list, np.ndarray)):  # (a0, a255): signal-dependent noise, the amplitude per byte from the value before the noise
        a0, a255 = (int(a) for a in noise)
        if min(a0, a255) < 0 or max(a0, a255) > 255:
            raise ValueError("noise is an amplitude in bytes, 0 .. 255, or a pair of them (at byte 0, at byte 255)")
        out = np.empty_like(frames)
        for j in range(frames.shape[0]):
            rng = np.random.default_rng([int(noise_seed), j])
            v = frames[j].astype(np.int64)
            amp = a0 + ((a255 - a0) * v + 127) // 255
            out[j] = np.clip(v + rng.integers(-amp, amp + 1), 0, 255).astype(np.uint8)
        return out
    if not noise:
        return frames
    noise = int(noise)
    if noise < 0 or noise > 255:
        raise ValueError("noise is an amplitude in bytes, 0 .. 255")
    out = np.empty_like(frames)
    for j in range(frames.shape[0]):
        rng = np.random.default_rng([int(noise_seed), j])
        out[j] = np.clip(frames[j].astype(np.int64) + rng.integers(-noise, noise + 1, size=frames[j].shape), 0, 255).astype(np.uint8)
    return out


def _mover_block(mover, seed):
    """the mover's bytes: render_occluded_pair's block texture ((h, w, 3) uint8), _texture in the block's own coordinates under another seed"""
    h, bw = int(mover[2]), int(mover[3])
    by, bx = np.mgrid[0:h, 0:bw].astype(np.float64)
    return np.rint(_texture(3.0 * bx, 3.0 * by, (seed ^ 0xB10C) & 0xFFFFFFFF)[..., ::-1]).astype(np.uint8)


def mover_planes(nframes, rows, cols, mover):
    """the footprints of render_sequence's mover = (y0, x0, h, w, dx, dy): (nframes, rows, cols) bool, frame j's rectangle of h x w pixels at
    (y0 + j dy, x0 + j dx).  The rectangle must lie inside every frame"""
    y0, x0, h, bw, dx, dy = (int(b) for b in mover)
    ys, xs = [y0, y0 + (nframes - 1) * dy], [x0, x0 + (nframes - 1) * dx]
    if h < 1 or bw < 1 or min(ys) < 0 or min(xs) < 0 or max(ys) + h > rows or max(xs) + bw > cols:
        raise ValueError("the mover must lie inside every frame")
    planes = np.zeros((nframes, rows, cols), dtype=bool)
    for j in range(nframes):
        planes[j, y0 + j * dy:y0 + j * dy + h, x0 + j * dx:x0 + j * dx + bw] = True
    return planes


def _with_mover(frames, mover, seed):
    """the frames with the mover's block pasted onto every one (a new array); None: the frames themselves"""
    if mover is None:
        return frames
    planes = mover_planes(frames.shape[0], frames.shape[1], frames.shape[2], mover)
    block = _mover_block(mover, seed)
    out = frames.copy()
    for j in range(frames.shape[0]):
        out[j][planes[j]] = block.reshape(-1, 3)
    return out


def _box_mean(frame, b):
    """a frame's rounded box mean over b (odd) columns, edges replicated"""
    cols = frame.shape[1]
    idx = np.clip(np.arange(-(b // 2), cols + b // 2), 0, cols - 1)
    padded = frame.astype(np.int64)[:, idx]
    total = sum(padded[:, d:d + cols] for d in range(b))
    return ((2 * total + b) // (2 * b)).astype(np.uint8)


def _box_blurred(frames, blur):
    """the frames with frame j replaced by its rounded box mean over blur[j] (odd) columns, edges replicated (a new array); an entry that is a
    sequence gives every ROW of the frame its own width (`rows` of them); None or all 1: the frames themselves"""
    if blur is None:
        return frames
    blur = list(blur)
    if len(blur) != frames.shape[0]:
        raise ValueError("blur needs one odd box width >= 1 per frame (nframes)")
    widths = [int(b) if np.ndim(b) == 0 else None for b in blur]
    if any(b is not None and (b < 1 or b % 2 == 0) for b in widths):
        raise ValueError("blur needs one odd box width >= 1 per frame (nframes)")
    per_row = {}
    for j, b in enumerate(blur):
        if widths[j] is None:
            r = np.asarray(b, dtype=np.int64).reshape(-1)
            if r.shape[0] != frames.shape[1] or (r < 1).any() or (r % 2 == 0).any():
                raise ValueError("a per-row blur entry needs one odd box width >= 1 per row (rows)")
            per_row[j] = r
    if not per_row and all(b == 1 for b in widths):
        return frames
    out = frames.copy()
    for j, b in enumerate(widths):
        if b is not None and b > 1:
            out[j] = _box_mean(frames[j], b)
        elif b is None:
            for w in np.unique(per_row[j]):
                if w > 1:
                    out[j][per_row[j] == w] = _box_mean(frames[j], int(w))[per_row[j] == w]
    return out


def render_sequence(nframes, rows, cols, K, v, w, k=0.0, gamma=0.8, seed=0x5EED0000, speeds=None, gains=None, noise=None, noise_seed=0x5EED0001, mover=None, blur=None):
    """nframes 8-bit BGR frames of render_pair's texture under a constant motion: frame j at pixel q shows T(inv^j(q)), where inv is
    render_pair's fixed-point inverse of the model flow F (p + F(p) = q), applied j times from the pixel grid.  Every consecutive pair
    (j, j + 1) therefore has the true flow F and the true (v, w, k); render_pair's border mask.  nframes = 2 gives render_pair's two
    frames bit for bit.  Returns (frames (nframes, rows, cols, 3) uint8, F (rows, cols, 2), mask).
    speeds: one factor per pair on v (nframes - 1 of them): pair j moves with (speeds[j] v, w, k) and has the model flow F_j of that
    motion; F is then (nframes - 1, rows, cols, 2) and the band of the mask is the widest pair's.  None: the frames of a constant motion,
    byte for byte what this function returned before it had the argument.
    gains: one exposure factor per frame (nframes of them): frame j = clip(rint(gains[j] texture)); the geometry is unchanged.  None: byte
    for byte what this function returns without the argument.
    noise: an amplitude in bytes: after the exposure gain every byte of frame j gets an integer drawn uniformly from [-noise, noise] by the
    generator seeded (noise_seed, j), clipped to 0 .. 255 -- seeded integer sensor noise, what the temporal denoise is for.  None (or 0): byte
    for byte what this function returns without the argument.  A pair (a0, a255): signal-dependent noise, what the noise curve is for -- the
    amplitude of a byte of value v (before the noise) is a0 + ((a255 - a0) v + 127) // 255, the generators seeded in the same way; an integer
    behaves exactly as before.
    mover: (y0, x0, h, w, dx, dy): a rectangle of h x w pixels with render_occluded_pair's block texture pasted onto frame j at
    (y0 + j dy, x0 + j dx), after the exposure gain and before the sensor noise -- something that moves through a static scene, what the clean
    plate is for; it must lie inside every frame and has no part in F or the mask (mover_planes gives its footprints).  None: byte for byte
    what this function returns without the argument.
    blur: one odd horizontal box width per frame (nframes of them): frame j becomes its rounded box mean over blur[j] columns with replicated
    edges, after the mover and before the sensor noise -- the blur of a shaken exposure, what the sharpness transfer is for; the geometry is
    unchanged.  An entry may be a sequence of `rows` odd widths, one per row: the smear of a rolling-shutter exposure, which varies down the
    frame (what the sharpness transfer per scanline band is for).  None or all 1: byte for byte what this function returns without the argument."""
    if nframes < 2:
        raise ValueError("a sequence has at least two frames")
    if gains is not None and len(gains) != nframes:
        raise ValueError("gains needs one factor per frame (nframes)")
    if speeds is not None:
        frames, flows, mask = _render_sequence_speeds(nframes, rows, cols, K, v, w, k, gamma, seed, speeds, gains)
        return _sensor_noise(_box_blurred(_with_mover(frames, mover, seed), blur), noise, noise_seed), flows, mask
    flow, _ = make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    frames = [_exposed(_texture(xx, yy, seed), None if gains is None else gains[0])]
    qx, qy = xx, yy
    for j in range(1, nframes):
        px, py = qx.copy(), qy.copy()
        for _ in range(50):  # render_pair's iteration, from the previous frame's positions
            F = _bilinear(flow, px, py)
            nx, ny = qx - F[..., 0], qy - F[..., 1]
            done = max(np.abs(nx - px).max(), np.abs(ny - py).max()) < 1e-9
            px, py = nx, ny
            if done:
                break
        qx, qy = px, py
        frames.append(_exposed(_texture(qx, qy, seed), None if gains is None else gains[j]))
    band = int(np.ceil(np.abs(flow).max())) + 5
    mask = np.zeros((rows, cols), dtype=bool)
    mask[band:rows - band, band:cols - band] = True
    return _sensor_noise(_box_blurred(_with_mover(np.stack(frames), mover, seed), blur), noise, noise_seed), np.ascontiguousarray(flow), mask


def _render_sequence_speeds(nframes, rows, cols, K, v, w, k, gamma, seed, speeds, gains=None):
    """render_sequence with one speed factor per pair: its loop, with the model flow of pair j - 1 in step j"""
    speeds = [float(s_) for s_ in speeds]
    if len(speeds) != nframes - 1:
        raise ValueError("speeds needs one factor per pair (nframes - 1)")
    flows = [make_flow(rows, cols, K, s_ * np.asarray(v, dtype=np.float64), w, k, gamma, _model_only=True)[0] for s_ in speeds]
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    frames = [_exposed(_texture(xx, yy, seed), None if gains is None else gains[0])]
    qx, qy = xx, yy
    for j in range(1, nframes):
        flow = flows[j - 1]
        px, py = qx.copy(), qy.copy()
        for _ in range(50):
            F = _bilinear(flow, px, py)
            nx, ny = qx - F[..., 0], qy - F[..., 1]
            done = max(np.abs(nx - px).max(), np.abs(ny - py).max()) < 1e-9
            px, py = nx, ny
            if done:
                break
        qx, qy = px, py
        frames.append(_exposed(_texture(qx, qy, seed), None if gains is None else gains[j]))
    band = int(np.ceil(max(np.abs(f).max() for f in flows))) + 5
    mask = np.zeros((rows, cols), dtype=bool)
    mask[band:rows - band, band:cols - band] = True
    return np.stack(frames), np.ascontiguousarray(np.stack(flows)), mask


def default_motion():
    """examples/README.md:20 first synthetic example: v = (0.03, 0.03, 0) * mean depth, w = (0, 0, 0.5 deg), k = 0."""
    return np.array([0.03, 0.03, 0.0]), np.array([0.0, 0.0, np.deg2rad(0.5)]), 0.0


def make_config(cfg, seed=None, v=None, w=None, k=None, rows=None, cols=None):
    """Inputs of one BASELINE.json config: flow image + flattened solver inputs + truth."""
    c = dict(CONFIGS[cfg])
    if rows is not None:
        c["rows"] = rows
    if cols is not None:
        c["cols"] = cols
    dv, dw, dk = default_motion()
    v = dv if v is None else v
    w = dw if w is None else w
    k = dk if k is None else k
    K = INTRINSICS[c["K"]]
    if rows is not None or cols is not None:  # keep the principal point centred for resized instances
        base_r, base_c = CONFIGS[cfg]["rows"], CONFIGS[cfg]["cols"]
        sc = c["cols"] / base_c
        K = (K[0] * sc, K[1] * sc, K[2] * sc, K[3] * (c["rows"] / base_r))
    seed = (0x5EED0000 + cfg) if seed is None else seed
    flow, truth = make_flow(c["rows"], c["cols"], K, v, w, k, c["gamma"], c["noise_px"], c["outliers"], seed)
    q, u, alpha, alpha_k, pix = flatten_numpy(flow, K, c["gamma"])
    return dict(flow_img=flow, q=q, u=u, alpha=alpha, alpha_k=alpha_k, pix=pix, truth=truth, rows=c["rows"],
                cols=c["cols"], K=K, gamma=c["gamma"])
