"""GPU: the seam blend (include/rsdsfm_stabilize_blend.h) bit for bit against its definition (tests/stabilize_blend_spec_numpy.py) in both
library builds, with guard bytes behind every plane -- the distance on sizes that are no multiple of a word and rows longer than a workgroup's
segment, the sums (one past 2^32), the layer call's three thread paths, every source byte and layer-mask value inside one dword, the gains'
clamps and switches, feather 1 without gain against rsdsfm_stabilize_window_frame_dev's own fill pass, the argument errors, one context shared
with the dense, stabilise, fill and crop calls -- and the clip call (rsdsfm_stabilize_video_blended_dev) byte for byte against the public
calls made one after another.  The clip is tests/test_gpu_stabilize.py's, built here."""
import numpy as np
import pytest

import link_spec_numpy as link
import stabilize_blend_cases as cases
import stabilize_blend_spec_numpy as spec
import stabilize_cases as stab_cases
import stabilize_crop_cases as crop_cases
import stabilize_spec_numpy as stab

pytestmark = pytest.mark.gpu

GUARD = 0xCD
M_N = link.rodrigues(np.array([-0.03, 0.04, -0.02]))  # tests/test_gpu_stabilize_crop.py's neighbour pose
m_N = np.array([-0.1, 0.05, -0.15])


def _guarded(torch, dev, a):
    """a's bytes on the device with 16 guard bytes behind them: (the view of a's shape, the guard)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + 16,), GUARD, dtype=torch.uint8, device=dev)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[:a.size].view(*a.shape), buf[a.size:]


def _clean(*guards):
    for g in guards:
        assert (g.cpu().numpy() == GUARD).all()


# ---------------------------------------------------------------------------------------------------
# the distance
# ---------------------------------------------------------------------------------------------------
def _distance(torch, s, mask, T):
    dev = torch.device("cuda", 0)
    (d_m, g_m), (d_d, g_d) = _guarded(torch, dev, mask), _guarded(torch, dev, np.full(mask.shape, 0xEE, dtype=np.uint8))
    torch.cuda.synchronize()
    s.seam_distance_dev(d_m.data_ptr(), mask.shape[0], mask.shape[1], T, d_d.data_ptr())
    s.synchronize()
    _clean(g_m, g_d)
    assert np.array_equal(d_m.cpu().numpy(), mask)  # only read
    return d_d.cpu().numpy()


_dist_expected = {}


def _dist_want(name, shape, seed, mask, T):
    key = (name, shape, seed, T)
    if key not in _dist_expected:
        _dist_expected[key] = spec.seam_distance(mask, T)
    return _dist_expected[key]


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_distance_equals_the_spec(rsdsfm, arith):
    """(3, 5), (7, 5), (33, 70): rows that do not start on a word and the byte tail; (40, 1100): a row longer than one workgroup's segment;
    T 1, 2, 16, 64: larger than either side of the small frames; all set: every byte T; all empty: every byte 0"""
    import torch

    assert rsdsfm.seam_distance_launches(96, 128) == 2
    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in cases.DISTANCE_SIZES:
            for name, mask in cases.distance_masks(*shape, seed=shape[0] + shape[1]):
                for T in cases.FEATHERS:
                    got = _distance(torch, s, mask, T)
                    assert np.array_equal(got, _dist_want(name, shape, 0, mask, T)), (shape, name, T)
                    if name == "set":
                        assert (got == T).all()
                    if name == "empty":
                        assert not got.any()
        m = cases.distance_masks(33, 70, 5)[4][1]
        assert np.array_equal(s.seam_distance(m), spec.seam_distance(m, 16))  # the host convenience; feather 0 = 16


# ---------------------------------------------------------------------------------------------------
# one layer
# ---------------------------------------------------------------------------------------------------
def _blend(torch, s, e, T, sid=5, gain=True, min_overlap=1, with_counts=True):
    """rsdsfm_seam_blend_layer_dev on guarded planes; the record and the counters have a guard word on either side"""
    dev = torch.device("cuda", 0)
    rows, cols = e["mask"].shape
    ch = 1 if e["image"].ndim == 2 else 3
    names = ("layer", "lmask", "dist", "image", "mask", "source")
    d = {k: _guarded(torch, dev, e[k]) for k in names}
    rec = torch.full((10,), -7, dtype=torch.int64, device=dev)
    cnt = torch.full((4,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s.seam_blend_layer_dev(d["layer"][0].data_ptr(), d["lmask"][0].data_ptr(), ch, rows, cols, d["dist"][0].data_ptr(), sid, d["image"][0].data_ptr(),
                           d["mask"][0].data_ptr(), d["source"][0].data_ptr(), rec[1:].data_ptr(), cnt[1:].data_ptr() if with_counts else None, feather=T, gain=gain,
                           min_overlap=min_overlap)
    s.synchronize()
    _clean(*[d[k][1] for k in names])
    for k in ("layer", "lmask", "dist"):
        assert np.array_equal(d[k][0].cpu().numpy(), e[k]), k  # only read
    r, c = rec.cpu().numpy(), cnt.cpu().numpy()
    assert r[0] == -7 and r[9] == -7 and c[0] == -7 and c[3] == -7 and (with_counts or (c == -7).all())
    return dict(image=d["image"][0].cpu().numpy(), mask=d["mask"][0].cpu().numpy(), source=d["source"][0].cpu().numpy(), sums=r[1:9].view(np.uint64).copy(),
                counts=(int(c[1]), int(c[2])) if with_counts else None)


def _blend_want(e, T, sid=5, gain=True, min_overlap=1):
    ch = 1 if e["image"].ndim == 2 else 3
    image, mask, source = e["image"].copy(), e["mask"].copy(), e["source"].copy()
    sums = spec.overlap_sums(image, source, e["layer"], e["lmask"])
    G = spec.gains(sums, ch, min_overlap, 0 if gain else 1)
    counts = spec.blend_layer(image, mask, source, e["dist"], T, e["layer"], e["lmask"], sid, G)
    return dict(image=image, mask=mask, source=source, sums=sums, counts=counts, gains=G)


def _same(got, want, counts=True):
    for k in ("image", "mask", "source", "sums"):
        assert np.array_equal(got[k], want[k]), k
    if counts:
        assert got["counts"] == want["counts"]


_layer_cases = {}


def _layer_case(shape, ch, T, sparse):
    key = (shape, ch, T, sparse)
    if key not in _layer_cases:
        e = cases.layer_case(shape[0], shape[1], ch, 11 * shape[0] + shape[1] + ch, T, sparse=sparse)
        _layer_cases[key] = (e, _blend_want(e, T))
    return _layer_cases[key]


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_sums_and_blend_equal_the_spec(rsdsfm, arith):
    """the distance test's sizes with 1 and 3 channels: the untouched path (a dword all T and sourced), the mixed path (source bytes 0, 1 and
    >= 2 and layer masks 0, 1 and 255 inside one dword) and the byte tail; counters present and absent"""
    import torch

    assert rsdsfm.seam_blend_layer_launches(96, 128) == 2
    seen = [0, 0]
    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in cases.DISTANCE_SIZES:
            for ch in (1, 3):
                for T, sparse in ((16, False), (4, True)):
                    e, want = _layer_case(shape, ch, T, sparse)
                    got = _blend(torch, s, e, T)
                    _same(got, want)
                    assert got["counts"][0] == int(got["mask"].sum()) - int(e["mask"].sum())
                    assert rsdsfm.seam_gains(got["sums"], ch, 1).tolist()[:ch] == want["gains"]
                    seen = [seen[0] + want["counts"][0], seen[1] + want["counts"][1]]
                e, want = _layer_case(shape, ch, 16, False)
                _same(_blend(torch, s, e, 16, with_counts=False), want, counts=False)
    assert min(seen) > 5000
    e, _ = _layer_case((96, 128), 3, 16, False)
    words = lambda a: a.reshape(-1, 4)
    untouched = (words(e["dist"]) == 16).all(axis=1) & (words(e["source"]) != 0).all(axis=1)
    kinds = np.stack([(words(e["source"]) == 0).any(axis=1), (words(e["source"]) == 1).any(axis=1), (words(e["source"]) >= 2).any(axis=1)]).all(axis=0)
    assert untouched.sum() > 500 and kinds.sum() > 5  # the paths the case is there for


def test_a_sum_past_thirty_two_bits(rsdsfm):
    """a gray plane of 4110 x 4110, all 255 under a full overlap: count = 4110^2 = 16892100, both sums 255 x 4110^2 = 4307485500 > 2^32; the
    gain is exactly 1 and, the distance being T everywhere, no byte changes"""
    import torch

    dev = torch.device("cuda", 0)
    n = 4110
    full = lambda v: torch.full((n, n), v, dtype=torch.uint8, device=dev)
    image, layer, mask, source, lmask, dist = full(255), full(255), full(1), full(1), full(1), full(16)
    rec, cnt = torch.full((8,), -1, dtype=torch.int64, device=dev), torch.full((2,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        s.seam_blend_layer_dev(layer.data_ptr(), lmask.data_ptr(), 1, n, n, dist.data_ptr(), 2, image.data_ptr(), mask.data_ptr(), source.data_ptr(), rec.data_ptr(),
                               cnt.data_ptr())
        s.synchronize()
    assert 255 * n * n == 4307485500 > 1 << 32
    assert rec.cpu().numpy().tolist() == [16892100, 4307485500, 4307485500, 0, 0, 0, 0, 0] and cnt.cpu().numpy().tolist() == [0, 0]
    assert rsdsfm.seam_gains(rec.cpu().numpy().view(np.uint64), 1).tolist() == [65536] * 3
    assert bool((image == 255).all()) and bool((source == 1).all()) and bool((mask == 1).all())


def test_gain_cases(rsdsfm):
    """the gain clamped at each end (a layer of 1s under an own frame of 255s, and the reverse), a layer of 0s (nothing to divide by), a count
    under min_overlap, the gain off: the spec's bytes and the host's gains from the record"""
    import torch

    base = cases.exposure_case(1.0, rows=33, cols=70, T=4)
    own = int(base["mask"].sum())
    runs = []
    for own_v, layer_v, kw, G in ((255, 1, {}, spec.GAIN_MAX), (1, 255, {}, spec.GAIN_MIN), (200, 0, {}, spec.GAIN_ONE), (100, 50, dict(min_overlap=own + 1), spec.GAIN_ONE),
                                  (100, 50, dict(min_overlap=own), 131072), (100, 50, dict(gain=False), spec.GAIN_ONE), (100, 50, dict(min_overlap=0), 131072)):
        e = dict(base, image=np.where(base["mask"] == 1, own_v, 0).astype(np.uint8), layer=np.full_like(base["image"], layer_v))
        runs.append((e, kw, G))
    with rsdsfm.Solver(0) as s:
        for e, kw, G in runs:
            spec_kw = dict(kw, min_overlap=kw.get("min_overlap", 1) or spec.MIN_OVERLAP_DEFAULT)
            want = _blend_want(e, 4, **spec_kw)
            assert want["gains"] == [G]
            got = _blend(torch, s, e, 4, **kw)
            _same(got, want)
            assert rsdsfm.seam_gains(got["sums"], 1, kw.get("min_overlap", 1), 0 if kw.get("gain", True) else 1).tolist() == [G, spec.GAIN_ONE, spec.GAIN_ONE]
    assert own >= spec.MIN_OVERLAP_DEFAULT


_pairs = {}


def _pair(oracle, shape, ch):
    """tests/test_gpu_stabilize_crop.py's pair: an own frame (the stabiliser's standard case, rendered by the spec) and a neighbour of other
    bytes and other holes"""
    if (shape, ch) not in _pairs:
        rows, cols = shape
        K, image, depth = crop_cases.inputs(rows, cols, channels=ch, holes=0.4)
        R, t = oracle.pose_table(crop_cases.POSE["v"], crop_cases.POSE["w"], crop_cases.POSE["k"], crop_cases.POSE["gamma"], rows)
        R = np.ascontiguousarray(R).reshape(rows, 9)
        nimage = np.ascontiguousarray(np.roll(image, (1, 2), axis=(0, 1))[::-1])
        ndepth = np.ascontiguousarray(np.roll(depth, (1, 2), axis=(0, 1)))
        own = stab.stabilize_frame(image, depth, R, t, K, stab_cases.M_STD, stab_cases.m_STD)
        _pairs[(shape, ch)] = dict(K=K, image=image, depth=depth, R=R, t=t, nimage=nimage, ndepth=ndepth, own=own)
    return _pairs[(shape, ch)]


def _window_call(torch, s, e, image, mask, source, window, sid=2, with_source=True):
    dev = torch.device("cuda", 0)
    rows, cols = mask.shape
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_n, d_dm, d_R, d_t = tt(e["nimage"]), tt(e["ndepth"].T), tt(e["R"]), tt(e["t"])
    (d_img, g0), (d_mask, g1), (d_src, g2) = _guarded(torch, dev, image), _guarded(torch, dev, mask), _guarded(torch, dev, source)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s.stabilize_window_frame_dev(d_n.data_ptr(), 1 if image.ndim == 2 else 3, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, M_N, m_N, sid, window,
                                 d_img.data_ptr(), d_mask.data_ptr(), d_src.data_ptr() if with_source else None, cnt.data_ptr())
    s.synchronize()
    _clean(g0, g1, g2)
    return dict(image=d_img.cpu().numpy(), mask=d_mask.cpu().numpy(), source=d_src.cpu().numpy(), count=int(cnt.cpu()[0]))


@pytest.mark.parametrize("shape,ch", [((33, 70), 3), ((96, 128), 1)])
def test_feather_one_without_gain_is_the_window_calls_fill_pass(oracle, rsdsfm, shape, ch):
    """the neighbour rendered alone onto a zeroed layer, then the layer call with T = 1 and the gain off on the own frame's planes: byte for
    byte rsdsfm_stabilize_window_frame_dev of the neighbour on those planes, and `filled` is its count"""
    import torch

    e = _pair(oracle, shape, ch)
    rows, cols = shape
    image, mask = e["own"]["image"], e["own"]["mask"]
    zero = np.zeros_like(mask)
    with rsdsfm.Solver(0) as s:
        for window in ((0, 0, rows, cols), (rows // 6, cols // 5, (2 * rows) // 3, ((2 * rows) // 3 * cols) // rows)):
            want = _window_call(torch, s, e, image, mask, mask, window)
            layer = _window_call(torch, s, e, np.zeros_like(image), zero, zero, window, with_source=False)
            dist = _distance(torch, s, mask, 1)
            assert np.array_equal(dist, (mask != 0).astype(np.uint8))
            got = _blend(torch, s, dict(image=image, mask=mask, source=mask, dist=dist, layer=layer["image"], lmask=layer["mask"]), 1, sid=2, gain=False)
            for k in ("image", "mask", "source"):
                assert np.array_equal(got[k], want[k]), (window, k)
            assert got["counts"] == (want["count"], 0) and want["count"] > 0


def test_argument_errors(rsdsfm):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    plane = lambda ch=1: torch.zeros(rows * cols * ch + 8, dtype=torch.uint8, device=dev)
    layer, lmask, dist, image, mask, source = plane(3), plane(), plane(), plane(3), plane(), plane()
    rec, cnt = torch.zeros(9, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    P = lambda t: t.data_ptr()
    with rsdsfm.Solver(0) as s:
        for bad in (dict(m=0), dict(d=0), dict(m=P(mask) + 1), dict(d=P(dist) + 2), dict(d=P(mask)), dict(r=1), dict(c=1), dict(r=16385), dict(c=16385), dict(T=65),
                    dict(T=-1)):
            kw = dict(dict(m=P(mask), r=rows, c=cols, T=16, d=P(dist)), **bad)
            with pytest.raises(rsdsfm.RsdsfmError):
                s.seam_distance_dev(kw["m"], kw["r"], kw["c"], kw["T"], kw["d"])
        s.seam_distance_dev(P(mask), rows, cols, 64, P(dist))  # the same arguments without a fault go through
        ok = dict(li=P(layer), lm=P(lmask), ch=3, r=rows, c=cols, d=P(dist), sid=2, i=P(image), m=P(mask), s=P(source), rec=P(rec), cnt=P(cnt), kw={})
        for bad in (dict(li=0), dict(lm=0), dict(d=0), dict(i=0), dict(m=0), dict(s=0), dict(rec=0), dict(li=P(layer) + 1), dict(lm=P(lmask) + 2), dict(d=P(dist) + 3),
                    dict(i=P(image) + 1), dict(m=P(mask) + 1), dict(s=P(source) + 2), dict(rec=P(rec) + 4), dict(cnt=P(cnt) + 4), dict(li=P(image)), dict(lm=P(mask)),
                    dict(lm=P(source)), dict(d=P(mask)), dict(d=P(source)), dict(s=P(mask)), dict(sid=0), dict(sid=1), dict(sid=256), dict(ch=2), dict(r=1), dict(c=1),
                    dict(r=16385), dict(c=16385), dict(kw=dict(feather=65)), dict(kw=dict(feather=-1)), dict(kw=dict(min_overlap=-1))):
            a = dict(ok, **bad)
            with pytest.raises(rsdsfm.RsdsfmError):
                s.seam_blend_layer_dev(a["li"], a["lm"], a["ch"], a["r"], a["c"], a["d"], a["sid"], a["i"], a["m"], a["s"], a["rec"], a["cnt"], **a["kw"])
        call = lambda p: s.lib.rsdsfm_seam_blend_layer_dev(s._ctx, rsdsfm._dp(P(layer)), rsdsfm._dp(P(lmask)), 3, rows, cols, rsdsfm._dp(P(dist)), p, 2, rsdsfm._dp(P(image)),
                                                           rsdsfm._dp(P(mask)), rsdsfm._dp(P(source)), rsdsfm._dp(P(rec)), None)
        assert call(rsdsfm.C.byref(rsdsfm.StabilizeBlendParams(0, 0, 0, 31))) == -1  # bad struct_bytes
        assert call(rsdsfm.C.byref(rsdsfm.StabilizeBlendParams(0, 0, 2, 32))) == -1  # bad gain_mode
        assert call(rsdsfm.C.byref(rsdsfm.StabilizeBlendParams(0, 0, 0, 0))) == 0 and call(None) == 0  # a zeroed struct and NULL: the defaults
        s.seam_blend_layer_dev(P(layer), P(lmask), 3, rows, cols, P(dist), 255, P(image), P(mask), P(source), P(rec), P(cnt), feather=64)
        s.synchronize()
    assert not image.any() and not mask.any() and cnt.cpu().numpy().tolist() == [0, 0, 0]  # an empty layer changes nothing


def test_blend_dense_stabilise_fill_and_crop_alternate_on_one_context(oracle, rsdsfm):
    """distance, blend, dense, stabilise, fill, window-search and window-frame calls at two sizes on ONE context (one workspace, rebuilt only
    when the size changes, the row pass's plane with it): the spec's result every time"""
    import torch

    import stabilize_crop_spec_numpy as crop_spec

    dev = torch.device("cuda", 0)
    a, b = _pair(oracle, (33, 70), 3), _pair(oracle, (96, 128), 1)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    with rsdsfm.Solver(0) as s:
        for e in (a, b, a):
            rows, cols = e["depth"].shape
            ch = 1 if e["image"].ndim == 2 else 3
            image, mask = e["own"]["image"], e["own"]["mask"]
            assert np.array_equal(_distance(torch, s, mask, 16), spec.seam_distance(mask, 16))
            d_img, d_dm, d_R, d_t = tt(e["image"]), tt(e["depth"].T), tt(e["R"]), tt(e["t"])
            out, d_mask = torch.full_like(d_img, 77), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            s.rectify_dense_frame_dev(d_img.data_ptr(), ch, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, out.data_ptr(), d_mask.data_ptr())
            s.stabilize_frame_dev(d_img.data_ptr(), ch, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, stab_cases.M_STD, stab_cases.m_STD,
                                  out.data_ptr(), d_mask.data_ptr())
            s.synchronize()
            assert np.array_equal(out.cpu().numpy(), image) and np.array_equal(d_mask.cpu().numpy(), mask)
            window = s.crop_window_dev([d_mask.data_ptr()], rows, cols, rows * cols // 50, 0)
            assert window == crop_spec.crop_window(mask[None], max_empty=rows * cols // 50, margin=0)
            layer = _window_call(torch, s, e, np.zeros_like(image), np.zeros_like(mask), np.zeros_like(mask), window, with_source=False)
            case = dict(image=image, mask=mask, source=mask, dist=_distance(torch, s, mask, 8), layer=layer["image"], lmask=layer["mask"])
            assert np.array_equal(case["dist"], spec.seam_distance(mask, 8))
            _same(_blend(torch, s, case, 8, min_overlap=64), _blend_want(case, 8, min_overlap=64))
            d_fill, d_fmask, d_n, d_ndm = tt(image), tt(mask), tt(e["nimage"]), tt(e["ndepth"].T)
            torch.cuda.synchronize()
            s.stabilize_fill_frame_dev(d_n.data_ptr(), ch, d_ndm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, M_N, m_N, 2,
                                       d_fill.data_ptr(), d_fmask.data_ptr())
            s.synchronize()
            full = _window_call(torch, s, e, image, mask, mask, (0, 0, rows, cols))
            assert np.array_equal(d_fill.cpu().numpy(), full["image"]) and np.array_equal(d_fmask.cpu().numpy(), full["mask"])


# ---------------------------------------------------------------------------------------------------
# the clip
# ---------------------------------------------------------------------------------------------------
TRIALS = 20


@pytest.fixture(scope="module")
def clip(rsdsfm):
    """tests/test_gpu_stabilize.py's clip: 5 frames of 96 x 128, built here"""
    rows, cols, gamma = 96, 128, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    sc = 3.0 / np.abs(f0).max()
    frames, _, _ = rsdsfm.synth.render_sequence(5, rows, cols, K, v * sc, w * sc, k, gamma, seed=21, speeds=(1.0, 1.4, 0.8, 1.0))
    return frames, rows, cols, K, gamma, [3 + 5 * i for i in range(4)]


def _clip_run(rsdsfm, torch, clip, channels, radius, window_in, host_arrays, one_call, feather=None, margin=0, max_empty=200):
    """the blended clip on a fresh context: rsdsfm_stabilize_video_blended_dev, or the cropped clip call and the loop of public calls"""
    frames, rows, cols, K, gamma, seeds = clip
    if channels == 1:
        frames = np.ascontiguousarray(frames[..., 1])
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)]
    planes = lambda value, like=None: [torch.full_like(d_frames[0], value) if like else torch.full((rows, cols), value, dtype=torch.uint8, device=dev) for _ in range(n)]
    d_stab, d_smask, d_source = planes(77, True), planes(77), planes(GUARD)
    d_crop, d_cmask, d_csource = planes(55, True), planes(55), planes(55)
    d_blend, d_bmask, d_bsource = planes(33, True), planes(33), planes(33)
    dms = [torch.zeros(rows * cols, dtype=torch.float64, device=dev) for _ in range(n)]
    Rs = [torch.zeros((rows, 9), dtype=torch.float64, device=dev) for _ in range(n)]
    ts = [torch.zeros((rows, 3), dtype=torch.float64, device=dev) for _ in range(n)]
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a]
    common = dict(window_in=window_in, max_empty=max_empty, margin=margin, d_sources=ptrs(d_source), fill_radius=radius, sigma=1.0, seeds=seeds, trials=TRIALS)
    head = (ptrs(d_frames), rows, cols, channels, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs), ptrs(ts), ptrs(d_stab), ptrs(d_smask), ptrs(d_crop), ptrs(d_cmask))
    with rsdsfm.Solver(0) as s:
        if one_call:
            r = s.stabilize_video_blended_dev(*head, ptrs(d_blend), ptrs(d_bmask), ptrs(d_bsource), blend_feather=feather, blend_min_overlap=64,
                                              want_gains=host_arrays, want_blend_counts=host_arrays, d_crop_sources=ptrs(d_csource), **common)
            s.synchronize()
        else:
            r = s.stabilize_video_cropped_dev(*head, ptrs(d_csource), **common)
            s.synchronize()
            d_dist = torch.full((rows, cols), 99, dtype=torch.uint8, device=dev)
            d_layer, d_lmask = torch.zeros_like(d_frames[0]), torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
            d_sums = torch.zeros((n, max(2 * radius, 1), 8), dtype=torch.int64, device=dev)
            d_cnt = torch.zeros((n, max(2 * radius, 1), 2), dtype=torch.int64, device=dev)
            d_own = torch.zeros(n, dtype=torch.int64, device=dev)
            for a in d_blend + d_bmask + d_bsource:
                a.zero_()
            torch.cuda.synchronize()
            for p in range(n if r["window"][2] else 0):
                s.stabilize_window_frame_dev(d_frames[p].data_ptr(), channels, dms[p].data_ptr(), Rs[p].data_ptr(), ts[p].data_ptr(), K, rows, cols, r["M"][p], r["m"][p], 1,
                                             r["window"], d_blend[p].data_ptr(), d_bmask[p].data_ptr(), d_bsource[p].data_ptr(), d_own[p:].data_ptr())
                s.seam_distance_dev(d_bmask[p].data_ptr(), rows, cols, feather or 0, d_dist.data_ptr())
                for q, sid, nM, nm in (list(zip(*rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p, radius))) if radius else []):
                    s.synchronize()
                    d_layer.zero_()
                    d_lmask.zero_()
                    torch.cuda.synchronize()
                    s.stabilize_window_frame_dev(d_frames[q].data_ptr(), channels, dms[q].data_ptr(), Rs[q].data_ptr(), ts[q].data_ptr(), K, rows, cols, nM, nm, int(sid),
                                                 r["window"], d_layer.data_ptr(), d_lmask.data_ptr(), None, None)
                    s.seam_blend_layer_dev(d_layer.data_ptr(), d_lmask.data_ptr(), channels, rows, cols, d_dist.data_ptr(), int(sid), d_blend[p].data_ptr(),
                                           d_bmask[p].data_ptr(), d_bsource[p].data_ptr(), d_sums[p, int(sid) - 2].data_ptr(), d_cnt[p, int(sid) - 2].data_ptr(),
                                           feather=feather, min_overlap=64)
            s.synchronize()
            sums, per, own = d_sums.cpu().numpy().view(np.uint64)[:, :2 * radius], d_cnt.cpu().numpy()[:, :2 * radius], d_own.cpu().numpy()
            r["gains"] = np.array([[rsdsfm.seam_gains(rec, channels, 64) for rec in frame] for frame in sums], dtype=np.uint32).reshape(n, 2 * radius, 3)
            r["blend_counts"] = np.concatenate([(rows * cols - own - per[:, :, 0].sum(axis=1))[:, None], (own - per[:, :, 1].sum(axis=1))[:, None], per.reshape(n, 4 * radius)],
                                               axis=1)
        host = lambda a: [t.cpu().numpy() for t in a]
        r.update(images=host(d_stab), crops=host(d_crop), crop_masks=host(d_cmask), crop_sources=host(d_csource), blends=host(d_blend), blend_masks=host(d_bmask),
                 blend_sources=host(d_bsource))
    return r


@pytest.mark.parametrize("channels,radius,window_in,host_arrays,feather", [(3, 2, None, True, None), (3, 0, (7, 11, 60, 80), True, 8), (1, 2, (0, 0, 96, 128), False, 4),
                                                                           (1, 1, None, True, 64)])
def test_blended_clip_equals_its_parts(rsdsfm, clip, channels, radius, window_in, host_arrays, feather):
    import torch

    want = _clip_run(rsdsfm, torch, clip, channels, radius, window_in, host_arrays, one_call=False, feather=feather)
    got = _clip_run(rsdsfm, torch, clip, channels, radius, window_in, host_arrays, one_call=True, feather=feather)
    npix = 96 * 128
    assert got["window"] == want["window"] and got["window"][2] >= 1
    for name in ("scales", "A", "c", "A_s", "c_s", "M", "m", "valid", "counts", "crop_counts") + (("gains", "blend_counts") if host_arrays else ()):
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name
    assert ("gains" in got) == host_arrays == ("blend_counts" in got)
    for p in range(4):
        for k in ("images", "crops", "crop_masks", "crop_sources", "blends", "blend_masks", "blend_sources"):
            assert np.array_equal(got[k][p], want[k][p]), (k, p)
        assert np.array_equal(got["blend_masks"][p], got["crop_masks"][p])  # the blend fills what the crop fills
        assert set(np.unique(got["blend_masks"][p])) <= {0, 1} and not got["blends"][p][got["blend_masks"][p] == 0].any()
        if radius == 0:
            assert np.array_equal(got["blends"][p], got["crops"][p]) and np.array_equal(got["blend_sources"][p], got["blend_masks"][p])
        if host_arrays:
            counts = got["blend_counts"][p]
            assert counts.shape == (2 + 4 * radius,) and counts.sum() == npix and counts[0] == (got["blend_masks"][p] == 0).sum()
            by_id = np.bincount(got["blend_sources"][p].reshape(-1), minlength=2 + 2 * radius)
            assert by_id[1] == counts[1] and by_id[2:].tolist() == (counts[2::2] + counts[3::2]).tolist()
            assert got["gains"].shape == (4, 2 * radius, 3) and (got["gains"] >= spec.GAIN_MIN).all() and (got["gains"] <= spec.GAIN_MAX).all()
    if host_arrays:
        print("window", got["window"], "blend counts", got["blend_counts"].tolist(), "gains", got["gains"].tolist())
        if radius:
            assert got["blend_counts"][:, 3::2].sum() > 0  # something was blended


def test_clip_argument_errors(rsdsfm, clip):
    import torch

    for bad in (dict(feather=65), dict(feather=-1), dict(window_in=(0, 0, 97, 128)), dict(radius=17)):
        kw = dict(dict(radius=1, window_in=None, feather=None), **bad)
        with pytest.raises(rsdsfm.RsdsfmError):
            _clip_run(rsdsfm, torch, clip, 3, kw["radius"], kw["window_in"], True, one_call=True, feather=kw["feather"])


def test_evaluate_real_sequence_with_blend(rsdsfm, clip, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, fill=2, crop=True, blend=True) and without crop: what it returned before, the blended frames
    where the crop's are except in the feather and by the gain, the files; its ValueErrors"""
    frames, rows, cols, K, gamma, seeds = clip
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, out_dir=str(tmp_path / "blend"), fill=2, crop=True, crop_margin=0, crop_max_empty=200, blend=True, blend_feather=8, **kw)
        plain = ev(s, frames, out_dir=str(tmp_path / "plain"), fill=2, crop=True, crop_margin=0, crop_max_empty=200, **kw)
        hard = ev(s, frames, fill=2, blend=True, blend_feather=1, blend_gain=False, **kw)
        for bad in (dict(fill=2, blend=True, stabilize=False), dict(blend=True), dict(fill=0, crop=True, blend=True)):
            with pytest.raises(ValueError):
                ev(s, frames, **dict(kw, **bad))
    new = {"stab_blended", "blend_gains", "blend_counts"}
    assert set(out) == set(plain) | new
    for name in ("scales", "A", "c", "broken", "stab_valid", "fill_counts", "crop_counts"):
        assert np.array_equal(np.asarray(out[name]), np.asarray(plain[name])), name
    assert out["crop_window"] == plain["crop_window"] and out["crop_window"][2] >= 1
    assert out["blend_counts"].shape == (4, 10) and out["blend_gains"].shape == (4, 4, 3) and out["blend_gains"].dtype == np.uint32
    for p in range(4):
        for k in ("stabilized", "stab_masks", "stab_filled", "stab_sources", "stab_cropped"):
            assert np.array_equal(out[k][p], plain[k][p]), (k, p)
        assert out["blend_counts"][p].sum() == rows * cols and out["blend_counts"][p][0] == out["crop_counts"][p][0]
        assert np.array_equal(rsdsfm.formats.read_png(str(tmp_path / "blend" / ("stabilized_blended_%d.png" % p))), out["stab_blended"][p])
        # feather 1 without gain through the full frame: the hard fill (the filled clip renders the own frame with the stabiliser's call,
        # whose bytes the full-frame window call reproduces)
        assert np.array_equal(hard["stab_blended"][p], hard["stab_filled"][p]) and (hard["blend_gains"][p] == spec.GAIN_ONE).all()
        assert hard["blend_counts"][p][3::2].sum() == 0 and hard["blend_counts"][p][2::2].tolist() == hard["fill_counts"][p][2:].tolist()
    lines = (tmp_path / "blend" / "blend.csv").read_text().strip().split("\n")
    assert lines[0].startswith("pair,none,own_untouched,prev1_filled,prev1_blended,next1_filled") and lines[0].endswith("gain_next2_2") and len(lines) == 5
    assert lines[1].split(",")[1:11] == [str(x) for x in out["blend_counts"][0]]
    assert sorted(x.name for x in (tmp_path / "plain").iterdir()) == sorted(x.name for x in (tmp_path / "blend").iterdir() if "blend" not in x.name)
