"""GPU: the crop's window (rsdsfm_crop_window_dev) and one frame through a window (rsdsfm_stabilize_window_frame_dev) bit for bit against
their definition (tests/stabilize_crop_spec_numpy.py) in both library builds -- the windows known exactly, planes of 1s and of 255s, sizes that
are no multiple of a word, a table past 16 bits, margins, random masks, guard bytes; the full-frame window against the fill's call, the exact
zoom, a 1 x 1 window, the search's own result, the starting masks that drive the kernel's three paths, special depths -- and the clip call
(rsdsfm_stabilize_video_cropped_dev) byte for byte against the public calls made one after another.  The clip is tests/test_gpu_stabilize.py's,
built here."""
import numpy as np
import pytest

import link_spec_numpy as link
import rectify_dense_spec_numpy as dense
import stabilize_cases as stab_cases
import stabilize_crop_cases as cases
import stabilize_crop_spec_numpy as spec
import stabilize_spec_numpy as stab

pytestmark = pytest.mark.gpu

M_N = link.rodrigues(np.array([-0.03, 0.04, -0.02]))  # tests/test_gpu_stabilize_fill.py's neighbour pose
m_N = np.array([-0.1, 0.05, -0.15])
SID = 2
GUARD = 0xCD
HOLES = dict(holes=0.4)


def _guarded(torch, dev, a):
    """a's bytes on the device with 16 guard bytes behind them: (the view of a's shape, the guard)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + 16,), GUARD, dtype=torch.uint8, device=dev)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[:a.size].view(*a.shape), buf[a.size:]


# ---------------------------------------------------------------------------------------------------
# the window
# ---------------------------------------------------------------------------------------------------
def _window(torch, s, masks, max_empty=0, margin=None):
    """crop_window_dev on guarded planes (padded so that every plane starts on a word): the planes and their guards are only read"""
    dev = torch.device("cuda", 0)
    planes = [_guarded(torch, dev, m) for m in masks]
    torch.cuda.synchronize()
    got = s.crop_window_dev([p.data_ptr() for p, _ in planes], masks[0].shape[0], masks[0].shape[1], max_empty, margin)
    for (p, g), m in zip(planes, masks):
        assert (g.cpu().numpy() == GUARD).all() and np.array_equal(p.cpu().numpy(), m)
    return got


def _spread(masks, planes, set_value):
    """the same AND from `planes` planes: every empty pixel is empty in one plane (chosen by its position), the set bytes are set_value"""
    common = spec.common_mask(masks)
    rows, cols = common.shape
    owner = (np.arange(rows * cols).reshape(rows, cols) * 7) % planes
    return [np.where(~common & (owner == k), 0, set_value).astype(np.uint8) for k in range(planes)]


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_exact_windows_on_the_device(rsdsfm, arith):
    import torch

    assert rsdsfm.crop_window_launches(96, 128) == 3
    with rsdsfm.Solver(0, arith=arith) as s:
        for name, masks, max_empty, margin, want in cases.exact_windows():
            assert spec.crop_window(masks, max_empty, margin) == want
            for planes, value in ((1, 1), (1, 255), (5, 255), (5, 1)):
                assert _window(torch, s, _spread(masks, planes, value), max_empty, margin) == want, (name, planes, value)
        assert s.crop_window(cases.exact_windows()[0][1], 0, 0) == (1, 8, 19, 31)  # the host convenience


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_windows_equal_the_spec(rsdsfm, arith):
    """sizes whose rows do not start on a word ((3, 5), (7, 5), (33, 70): the byte path and the byte tail), several workgroups and tiles of
    the row scan ((40, 1100): more than 1024 columns, a carry), margins 0, 1, 3, max_empty, 1 and 5 planes, random masks"""
    import torch

    with rsdsfm.Solver(0, arith=arith) as s:
        n = 0
        for (rows, cols), empty in (((3, 5), 0.1), ((7, 5), 0.05), ((33, 70), 0.01), ((96, 128), 0.05), ((96, 128), 0.002), ((40, 1100), 0.0005), ((2, 2), 0.0)):
            for planes, margin, max_empty in ((1, 0, 0), (5, 1, 0), (5, 3, 0), (1, 1, 3)):
                masks = list(cases.random_masks(rows, cols, planes, empty / planes, 100 * rows + planes + margin, set_value=255 if margin == 1 else 1))
                want = spec.crop_window(masks, max_empty, margin)
                assert _window(torch, s, masks, max_empty, margin) == want, (rows, cols, planes, margin, max_empty)
                n += want[2] > 0
        assert n >= 20
        assert _window(torch, s, list(cases.random_masks(96, 128, 2, 0.001, 5))) == spec.crop_window(cases.random_masks(96, 128, 2, 0.001, 5), 0, 1)  # margin None = 1


def test_a_table_past_sixteen_bits(rsdsfm):
    """(300, 400) all empty with max_empty = 120000: the table's last entry is 120000 > 65535 and the window is the frame; one empty less
    allowed and it is not"""
    import torch

    z = [np.zeros((300, 400), dtype=np.uint8)]
    with rsdsfm.Solver(0) as s:
        assert _window(torch, s, z, 120000, 1) == (0, 0, 300, 400)
        assert _window(torch, s, z, 119999, 0) == spec.crop_window(z, 119999, 0) != (0, 0, 300, 400)
        assert _window(torch, s, z, 0, 0) == (0, 0, 0, 0)


def test_window_argument_errors(rsdsfm):
    import torch

    dev = torch.device("cuda", 0)
    m = torch.ones((16, 68), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        for bad in (dict(rows=1), dict(cols=1), dict(rows=16385), dict(margin=65), dict(margin=-1), dict(max_empty=-1), dict(max_empty=16 * 64 + 1),
                    dict(planes=[m.data_ptr() + 1]), dict(planes=[0]), dict(planes=[]), dict(planes=[m.data_ptr(), 0])):
            kw = dict(dict(planes=[m.data_ptr()], rows=16, cols=64, max_empty=0, margin=1), **bad)
            with pytest.raises(rsdsfm.RsdsfmError):
                s.crop_window_dev(kw["planes"], kw["rows"], kw["cols"], kw["max_empty"], kw["margin"])
        assert s.crop_window_dev([m.data_ptr()], 16, 64, 16 * 64, 64) == (0, 0, 16, 64)
        p = rsdsfm.StabilizeCropParams(0, 1, 31)
        w = (rsdsfm.C.c_int32 * 4)()
        assert s.lib.rsdsfm_crop_window_dev(s._ctx, rsdsfm._ptr_array([m.data_ptr()]), 1, 16, 64, rsdsfm.C.byref(p), w) == -1  # bad struct_bytes
        assert s.lib.rsdsfm_crop_window_dev(s._ctx, rsdsfm._ptr_array([m.data_ptr()]), 1, 16, 64, None, None) == -1


# ---------------------------------------------------------------------------------------------------
# one frame through a window
# ---------------------------------------------------------------------------------------------------
SHAPES = [(2, 2), (3, 5), (24, 40), (33, 70), (96, 128)]
CASES = [(shape, ch, 0, 0, 0, "reference", HOLES) for shape in SHAPES for ch in (3, 1)]
CASES += [((33, 70), 3, it, 0, 0, "reference", HOLES) for it in (1, 3)]
CASES += [((33, 70), 3, 0, mode, q5, "reference", HOLES) for mode, q5 in ((0, 1), (1, 0))]
CASES += [((33, 70), 3, 0, 0, 0, "fused", HOLES), ((96, 128), 1, 0, 0, 0, "fused", HOLES)]
CASES += [((33, 70), 3, 0, 0, 0, "reference", dict(holes=0.4, specials=True)),                      # NaN, +-inf, negative and 1e308 depths
          ((33, 70), 1, 0, 0, 0, "reference", dict(holes=0.7, block=(8, 20, 10, 14), corner=(5, 9)))]  # a thinner map

_expected = {}


def _pair(oracle, shape, ch, it, mode, q5, nkw):
    """an own frame (the stabiliser's standard case) and a neighbour of other bytes and other holes (tests/test_gpu_stabilize_fill.py's pair),
    with the spec's own frame, computed once per case and shared; the candidates per window are added as they are asked for"""
    key = (shape, ch, it, mode, q5, tuple(sorted(nkw.items())))
    if key not in _expected:
        rows, cols = shape
        K, image, depth = cases.inputs(rows, cols, channels=ch, holes=0.4)
        _, _, ndepth = cases.inputs(rows, cols, channels=ch, **nkw)
        R, t = oracle.pose_table(cases.POSE["v"], cases.POSE["w"], cases.POSE["k"], cases.POSE["gamma"], rows)
        R = np.ascontiguousarray(R).reshape(rows, 9)
        nimage = np.ascontiguousarray(np.roll(image, (1, 2), axis=(0, 1))[::-1])
        ndepth = np.ascontiguousarray(np.roll(ndepth, (1, 2), axis=(0, 1)))
        own = stab.stabilize_frame(image, depth, R, t, K, stab_cases.M_STD, stab_cases.m_STD, mode=mode, q5_mode=q5, iterations=it)
        _expected[key] = dict(K=K, image=image, depth=depth, R=R, t=t, nimage=nimage, ndepth=ndepth, own=own, cands={}, modes=(it, mode, q5))
    return _expected[key]


def _cand(e, window):
    if window not in e["cands"]:
        it, mode, q5 = e["modes"]
        e["cands"][window] = spec.stabilize_frame_window(e["nimage"], e["ndepth"], e["R"], e["t"], e["K"], M_N, m_N, window, mode=mode, q5_mode=q5, iterations=it)
    return e["cands"][window]


def _want(cand, image, mask, source, sid=SID):
    take = (mask == 0) & (cand["mask"] == 1)
    out, m2, s2 = image.copy(), mask.copy(), source.copy()
    out[take] = cand["image"][take]
    m2[take] = 1
    s2[take] = sid
    return dict(image=out, mask=m2, source=s2, count=int(take.sum()))


def _render(torch, s, e, image, mask, source, window, nimage=None, ndepth=None, M=M_N, m=m_N, sid=SID, with_source=True, with_count=True, fill_call=False):
    """one window call (or, fill_call, one rsdsfm_stabilize_fill_frame_dev) on the given in-out planes (host arrays); every plane has guard
    bytes behind it and the counter a guard on either side"""
    dev = torch.device("cuda", 0)
    rows, cols = mask.shape
    it, mode, q5 = e.get("modes", (0, 0, 0))
    ch = 1 if image.ndim == 2 else 3
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_n, d_dm = tt(e["nimage"] if nimage is None else nimage), tt((e["ndepth"] if ndepth is None else ndepth).T)
    d_R, d_t = tt(e["R"]), tt(e["t"])
    (d_img, g_img), (d_mask, g_mask), (d_src, g_src) = _guarded(torch, dev, image), _guarded(torch, dev, mask), _guarded(torch, dev, source)
    cnt = torch.full((3,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    head = (d_n.data_ptr(), ch, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, M, m, sid)
    tail = (d_img.data_ptr(), d_mask.data_ptr(), d_src.data_ptr() if with_source else None, cnt[1:].data_ptr() if with_count else None)
    if fill_call:
        s.stabilize_fill_frame_dev(*head, *tail, mode=mode, q5_mode=q5, iterations=it)
    else:
        s.stabilize_window_frame_dev(*head, window, *tail, mode=mode, q5_mode=q5, iterations=it)
    s.synchronize()
    for g in (g_img, g_mask, g_src):
        assert (g.cpu().numpy() == GUARD).all()
    c = cnt.cpu().numpy().tolist()
    assert c[0] == -1 and c[2] == -1
    return dict(image=d_img.cpu().numpy(), mask=d_mask.cpu().numpy(), source=d_src.cpu().numpy(), count=c[1])


def _same(got, want):
    for k in ("image", "mask", "source"):
        assert np.array_equal(got[k], want[k]), k
    assert got["count"] == want["count"]


def _windows(shape, own_mask):
    """the full frame, a window inside it, a 1 x 1 window and the search's own result on the own mask"""
    rows, cols = shape
    inner = (rows // 6, cols // 5, max((2 * rows) // 3, 1), max(((2 * rows) // 3 * cols) // rows, 1))
    found = spec.crop_window(own_mask[None], max_empty=own_mask.size // 50, margin=0)
    return [w for w in dict.fromkeys([(0, 0, rows, cols), inner, (rows - 1, cols // 2, 1, 1), found]) if w[2] >= 1]


@pytest.mark.parametrize("shape,ch,it,mode,q5,arith,nkw", CASES)
def test_window_call_equals_the_spec(oracle, rsdsfm, shape, ch, it, mode, q5, arith, nkw):
    """on the own frame's planes (the stabiliser's standard case) the neighbour through every window; the count equals the mask's change; with
    the full frame every byte is rsdsfm_stabilize_fill_frame_dev's"""
    import torch

    e = _pair(oracle, shape, ch, it, mode, q5, nkw)
    assert rsdsfm.stabilize_window_launches(*shape) == rsdsfm.stabilize_fill_launches(*shape)
    image, mask = e["own"]["image"], e["own"]["mask"]
    zero = np.zeros_like(mask)
    with rsdsfm.Solver(0, arith=arith) as s:
        for window in _windows(shape, mask):
            got = _render(torch, s, e, image, mask, mask, window)
            _same(got, _want(_cand(e, window), image, mask, mask))
            assert got["count"] == int(got["mask"].sum()) - int(mask.sum())
            if window == (0, 0) + shape:
                _same(got, _render(torch, s, e, image, mask, mask, None, fill_call=True))
        window = _windows(shape, mask)[-1]  # the own frame itself, id 1, onto zeroed planes: the windowed stabiliser
        own_w = spec.stabilize_frame_window(e["image"], e["depth"], e["R"], e["t"], e["K"], stab_cases.M_STD, stab_cases.m_STD, window, mode=mode, q5_mode=q5, iterations=it)
        got = _render(torch, s, e, np.zeros_like(image), zero, zero, window, nimage=e["image"], ndepth=e["depth"], M=stab_cases.M_STD, m=stab_cases.m_STD, sid=1)
        _same(got, dict(image=own_w["image"], mask=own_w["mask"], source=own_w["mask"], count=own_w["valid"]))


@pytest.mark.parametrize("shape,ch", [((3, 5), 3), ((33, 70), 3), ((33, 70), 1), ((24, 40), 1)])
def test_starting_masks(oracle, rsdsfm, shape, ch):
    """all 1: no byte changes and the count is 0; all 0: the candidate exactly where it is valid; every pattern of the 4 bytes of a word: the
    read-modify-write path"""
    import torch

    e = _pair(oracle, shape, ch, 0, 0, 0, HOLES)
    rows, cols = shape
    window = (rows // 6, cols // 5, (2 * rows) // 3, ((2 * rows) // 3 * cols) // rows)
    cand = _cand(e, window)
    rng = np.random.default_rng(5)
    image = rng.integers(0, 256, size=e["image"].shape, dtype=np.uint8)
    source = rng.integers(6, 200, size=shape, dtype=np.uint8)
    pattern = ((np.arange(rows * cols) // 4 % 16) >> (np.arange(rows * cols) % 4) & 1).astype(np.uint8).reshape(shape)
    with rsdsfm.Solver(0) as s:
        ones = _render(torch, s, e, image, np.ones(shape, dtype=np.uint8), source, window)
        assert np.array_equal(ones["image"], image) and ones["mask"].all() and np.array_equal(ones["source"], source) and ones["count"] == 0
        zeros = _render(torch, s, e, image, np.zeros(shape, dtype=np.uint8), source, window)
        _same(zeros, _want(cand, image, np.zeros(shape, dtype=np.uint8), source))
        assert np.array_equal(zeros["mask"], cand["mask"]) and zeros["count"] == cand["valid"]
        _same(_render(torch, s, e, image, pattern, source, window), _want(cand, image, pattern, source))
        _same(_render(torch, s, e, image, 1 - pattern, source, window), _want(cand, image, 1 - pattern, source))
    if rows * cols > 900:  # (inside the frame the candidate may offer every pixel of the window)
        assert 0 < _want(cand, image, pattern, source)["count"] <= (pattern == 0).sum()


def test_exact_zoom_on_the_device(rsdsfm):
    """the shift case through (4, 14, 12, 20): the bytes are the image's bilinear samples at exactly 6 + ix / 2 - 0.25, 8 + iy / 2 - 0.25"""
    import torch

    z = cases.zoom2_case()
    e = dict(z, nimage=z["image"], ndepth=z["depth"])
    zero = np.zeros((24, 40), dtype=np.uint8)
    want = dense.saturate_u8(dense.bilinear(z["image"], z["px"], z["py"]))
    with rsdsfm.Solver(0) as s:
        for it in (1, 3):
            e["modes"] = (it, 0, 0)
            got = _render(torch, s, e, np.zeros_like(z["image"]), zero, zero, z["window"], M=z["M"], m=z["m"], sid=1)
            assert np.array_equal(got["image"], want) and got["mask"].all() and (got["source"] == 1).all() and got["count"] == 960
        e["modes"] = (0, 0, 0)
        full = _render(torch, s, e, np.zeros_like(z["image"]), zero, zero, (0, 0, 24, 40), M=z["M"], m=z["m"], sid=1)
        assert np.array_equal(full["image"], z["want"]) and np.array_equal(full["mask"], z["mask"]) and full["count"] == 640
        # the host convenience on a clip of one pair: zeroed planes, the own frame, no neighbour
        A, c = np.stack([np.eye(3)] * 2), np.zeros((2, 3))
        img, mask, source, counts = s.stabilize_cropped([z["image"]], [z["depth"]], [z["R"]], [z["t"]], z["K"], A, c, A, c, np.ones(1), 0, z["M"], z["m"], z["window"],
                                                        radius=0)
        assert np.array_equal(img, want) and mask.all() and counts.tolist() == [0, 960]


def test_a_candidate_without_a_valid_depth_changes_nothing(oracle, rsdsfm):
    import torch

    e = _pair(oracle, (33, 70), 3, 0, 0, 0, HOLES)
    _, _, none_valid = cases.inputs(33, 70, none_valid=True)
    image, mask = e["own"]["image"], e["own"]["mask"]
    untouched = np.full(mask.shape, GUARD, dtype=np.uint8)
    with rsdsfm.Solver(0) as s:
        got = _render(torch, s, e, image, mask, mask, (3, 5, 20, 42), ndepth=none_valid)
        assert np.array_equal(got["image"], image) and np.array_equal(got["mask"], mask) and np.array_equal(got["source"], mask) and got["count"] == 0
        want = _want(_cand(e, (3, 5, 20, 42)), image, mask, mask)
        for with_source, with_count in ((False, False), (False, True), (True, False)):  # the optional outputs
            got = _render(torch, s, e, image, mask, mask if with_source else untouched, (3, 5, 20, 42), with_source=with_source, with_count=with_count)
            assert np.array_equal(got["image"], want["image"]) and np.array_equal(got["mask"], want["mask"])
            assert np.array_equal(got["source"], want["source"] if with_source else untouched) and got["count"] == (want["count"] if with_count else -1)


def test_neighbours_in_sequence_through_the_window(oracle, rsdsfm):
    """Solver.stabilize_cropped: the own call and one window call per candidate, against stabilize_cropped_frame (the golden fixture's case)"""
    g = np.load(cases.__file__.replace("stabilize_crop_cases.py", "golden/golden_stabilize_crop_v1.npz"))
    cc = cases.clip_case(oracle.pose_table, 33, 70, channels=3)
    window = tuple(int(x) for x in g["33x70/window"])
    with rsdsfm.Solver(0) as s:
        img, mask, source, counts = s.stabilize_cropped(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], 1,
                                                        cc["M"][1], cc["m"][1], window, radius=2)
    assert np.array_equal(img, g["33x70/out_image"]) and np.array_equal(mask, g["33x70/out_mask"]) and np.array_equal(source, g["33x70/out_source"])
    assert counts.tolist() == g["33x70/out_counts"].tolist()


def test_frame_argument_errors(rsdsfm):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    img = torch.zeros((rows, cols, 3), dtype=torch.uint8, device=dev)
    out = torch.zeros_like(img)
    mask, source = torch.zeros((rows, cols + 4), dtype=torch.uint8, device=dev), torch.zeros((rows, cols + 4), dtype=torch.uint8, device=dev)
    filled = torch.zeros(2, dtype=torch.int64, device=dev)
    dm, t = torch.ones(rows * cols, dtype=torch.float64, device=dev), torch.zeros(rows * 3, dtype=torch.float64, device=dev)
    R = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 9).repeat(rows, 1).contiguous()
    K = (50.0, 50.0, 32.0, 8.0)
    nanM = np.eye(3)
    nanM[1, 2] = np.nan
    with rsdsfm.Solver(0) as s:
        call = lambda i=img.data_ptr(), ch=3, d=dm.data_ptr(), o=out.data_ptr(), r=rows, c=cols, M=np.eye(3), m=np.zeros(3), sid=1, w=(2, 8, 8, 32), k=mask.data_ptr(), **kw: \
            s.stabilize_window_frame_dev(i, ch, d, R.data_ptr(), t.data_ptr(), K, r, c, M, m, sid, w, o, k, **kw)
        for bad in (dict(w=None), dict(w=(0, 0, 0, 32)), dict(w=(0, 0, 8, 0)), dict(w=(-1, 0, 8, 32)), dict(w=(0, -1, 8, 32)), dict(w=(9, 0, 8, 32)),
                    dict(w=(0, 33, 8, 32)), dict(w=(0, 0, 17, 64)), dict(M=None), dict(M=nanM), dict(o=img.data_ptr()), dict(d_source=mask.data_ptr()), dict(o=0),
                    dict(k=0), dict(ch=2), dict(mode=2), dict(iterations=17), dict(r=1), dict(sid=0), dict(sid=256), dict(o=out.data_ptr() + 1),
                    dict(d_filled=filled.data_ptr() + 4)):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        call(sid=255, w=(15, 63, 1, 1), d_source=source.data_ptr(), d_filled=filled.data_ptr())  # the same arguments without a fault go through
        s.synchronize()
    assert int(filled.cpu()[0]) == rows * cols  # constant depth, identity poses: every pixel of the empty mask is taken


def test_dense_stabilise_fill_and_crop_alternate_on_one_context(oracle, rsdsfm):
    """dense, stabilise, fill, window-search and window-frame calls at two sizes on ONE context (one workspace, rebuilt only when the size
    changes, the table with it): the spec's result every time"""
    import torch

    dev = torch.device("cuda", 0)
    a, b = _pair(oracle, (33, 70), 3, 0, 0, 0, HOLES), _pair(oracle, (96, 128), 1, 0, 0, 0, HOLES)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    with rsdsfm.Solver(0) as s:
        for e in (a, b, a):
            rows, cols = e["depth"].shape
            image, mask = e["own"]["image"], e["own"]["mask"]
            want_window = spec.crop_window(mask[None], max_empty=rows * cols // 50, margin=0)
            assert _window(torch, s, [mask], rows * cols // 50, 0) == want_window
            d_img, d_dm, d_R, d_t = tt(e["image"]), tt(e["depth"].T), tt(e["R"]), tt(e["t"])
            out, d_mask = torch.full_like(d_img, 77), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            s.rectify_dense_frame_dev(d_img.data_ptr(), 1 if e["image"].ndim == 2 else 3, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols,
                                      out.data_ptr(), d_mask.data_ptr())
            s.stabilize_frame_dev(d_img.data_ptr(), 1 if e["image"].ndim == 2 else 3, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols,
                                  stab_cases.M_STD, stab_cases.m_STD, out.data_ptr(), d_mask.data_ptr())
            s.synchronize()
            assert np.array_equal(out.cpu().numpy(), image) and np.array_equal(d_mask.cpu().numpy(), mask)
            assert s.crop_window_dev([d_mask.data_ptr()], rows, cols, rows * cols // 50, 0) == want_window
            _same(_render(torch, s, e, image, mask, mask, want_window), _want(_cand(e, want_window), image, mask, mask))
            _same(_render(torch, s, e, image, mask, mask, None, fill_call=True), _want(_cand(e, (0, 0, rows, cols)), image, mask, mask))
            assert _window(torch, s, [mask], 0, 1) == spec.crop_window(mask[None], 0, 1)


# ---------------------------------------------------------------------------------------------------
# the clip
# ---------------------------------------------------------------------------------------------------
TRIALS = 20


def _record(r, dm, R, t):
    sm = r["refine_summary"]
    return (r["n"], r["num_inliers"], r["best_trial"], r["flipped"], r["ransac_v"].tobytes(), r["ransac_w"].tobytes(), float(r["ransac_k"]), r["v"].tobytes(),
            r["w"].tobytes(), float(r["k"]), sm["num_iterations"], sm["num_successful_steps"], sm["termination"], sm["final_cost"], dm.cpu().numpy().tobytes(),
            R.cpu().numpy().tobytes(), t.cpu().numpy().tobytes())


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


def _clip_run(rsdsfm, torch, clip, batch, fused, radius, window_in, one_call, margin=1, max_empty=0):
    """the cropped clip on a fresh context: rsdsfm_stabilize_video_cropped_dev, or the inner clip call and the loop of public calls"""
    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)]
    d_fused = [torch.full((rows * cols,), np.nan, dtype=torch.float64, device=dev) for _ in range(n)] if fused else None
    planes = lambda value, like=None: [torch.full_like(d_frames[0], value) if like else torch.full((rows, cols), value, dtype=torch.uint8, device=dev) for _ in range(n)]
    d_stab, d_smask, d_source = planes(77, True), planes(77), planes(GUARD)
    d_crop, d_cmask, d_csource = planes(55, True), planes(55), planes(55)
    dms = [torch.zeros(rows * cols, dtype=torch.float64, device=dev) for _ in range(n)]
    Rs = [torch.zeros((rows, 9), dtype=torch.float64, device=dev) for _ in range(n)]
    ts = [torch.zeros((rows, 3), dtype=torch.float64, device=dev) for _ in range(n)]
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a] if a is not None else None
    common = dict(d_fused=ptrs(d_fused), sigma=1.0, seeds=seeds, trials=TRIALS)
    head = (ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs), ptrs(ts), ptrs(d_stab), ptrs(d_smask))
    with rsdsfm.Solver(0) as s:
        if batch:
            s.set_flow_batch(batch)
        if one_call:
            r = s.stabilize_video_cropped_dev(*head, ptrs(d_crop), ptrs(d_cmask), ptrs(d_csource), window_in=window_in, max_empty=max_empty, margin=margin,
                                              d_sources=ptrs(d_source), fill_radius=radius, **common)
            s.synchronize()
        else:
            if radius:
                r = s.stabilize_video_filled_dev(*head, ptrs(d_source), fill_radius=radius, **common)
            else:
                r = s.stabilize_video_dev(*head, **common)
                r["counts"] = np.stack([rows * cols - r["valid"], r["valid"]], axis=1)
            s.synchronize()
            r["window"] = tuple(window_in) if window_in else s.crop_window_dev(ptrs(d_smask), rows, cols, max_empty, margin)
            d_cnt = torch.zeros((n, 2 + 2 * radius), dtype=torch.int64, device=dev)
            for a in d_crop + d_cmask + d_csource:
                a.zero_()
            torch.cuda.synchronize()
            src = d_fused if fused else dms
            for p in range(n if r["window"][2] else 0):
                cand = [(p, 1, r["M"][p], r["m"][p])]
                if radius:
                    cand += list(zip(*rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p, radius)))
                for q, sid, nM, nm in cand:
                    s.stabilize_window_frame_dev(d_frames[q].data_ptr(), 3, src[q].data_ptr(), Rs[q].data_ptr(), ts[q].data_ptr(), K, rows, cols, nM, nm, int(sid),
                                                 r["window"], d_crop[p].data_ptr(), d_cmask[p].data_ptr(), d_csource[p].data_ptr(), d_cnt[p, int(sid):].data_ptr())
            s.synchronize()
            r["crop_counts"] = d_cnt.cpu().numpy()
            r["crop_counts"][:, 0] = rows * cols - r["crop_counts"][:, 1:].sum(axis=1)
        host = lambda a: [t.cpu().numpy() for t in a]
        r.update(records=[_record(x, dms[i], Rs[i], ts[i]) for i, x in enumerate(r["pairs"])], images=host(d_stab), masks=host(d_smask), sources=host(d_source),
                 crops=host(d_crop), crop_masks=host(d_cmask), crop_sources=host(d_csource), fused=host(d_fused) if fused else None)
    return r


@pytest.mark.parametrize("batch,fused,radius,window_in", [(1, False, 2, None), (0, False, 2, None), (0, True, 2, None), (0, False, 0, None),
                                                          (0, False, 2, (7, 11, 60, 80))])
def test_cropped_clip_equals_its_parts(rsdsfm, clip, batch, fused, radius, window_in):
    import torch

    want = _clip_run(rsdsfm, torch, clip, batch, fused, radius, window_in, one_call=False)
    got = _clip_run(rsdsfm, torch, clip, batch, fused, radius, window_in, one_call=True)
    npix = 96 * 128
    assert got["records"] == want["records"] and got["window"] == want["window"] and got["window"][2] >= 1
    if window_in:
        assert got["window"] == window_in
    for name in ("scales", "A", "c", "broken", "A_s", "c_s", "M", "m", "valid", "counts", "crop_counts"):
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name
    assert got["crop_counts"].shape == got["counts"].shape == (4, 2 + 2 * radius)
    for p in range(4):
        for k in ("images", "masks", "crops", "crop_masks", "crop_sources") + (("sources",) if radius else ()):
            assert np.array_equal(got[k][p], want[k][p]), (k, p)
        if not radius:
            assert (got["sources"][p] == GUARD).all()  # at radius 0 the inner call is the stabiliser's: no source plane
        counts = got["crop_counts"][p]
        assert set(np.unique(got["crop_masks"][p])) <= {0, 1} and counts.sum() == npix and counts[0] == (got["crop_masks"][p] == 0).sum()
        assert np.bincount(got["crop_sources"][p].reshape(-1), minlength=2 + 2 * radius).tolist() == counts.tolist()
        assert not got["crops"][p][got["crop_masks"][p] == 0].any()
        if fused:
            assert got["fused"][p].tobytes() == want["fused"][p].tobytes(), p
    print("window", got["window"], "crop counts", got["crop_counts"].tolist(), "counts", got["counts"].tolist())


def test_a_clip_without_a_window_and_argument_errors(rsdsfm, clip):
    """margin 64 and no empty pixel allowed: nothing fits a solved clip's masks; the crop planes are zeroed and none = rows cols"""
    import torch

    got = _clip_run(rsdsfm, torch, clip, 0, False, 1, None, one_call=True, margin=64, max_empty=0)
    if got["window"] == (0, 0, 0, 0):  # (what a solved clip's masks hold depends on the solve)
        assert got["crop_counts"].tolist() == [[96 * 128, 0, 0, 0]] * 4
        assert not any(a.any() for k in ("crops", "crop_masks", "crop_sources") for a in got[k])
    for bad in (dict(window_in=(0, 0, 97, 128)), dict(window_in=(0, 0, 0, 0)), dict(radius=17), dict(margin=65), dict(max_empty=-1)):
        kw = dict(dict(radius=1, window_in=None, margin=0, max_empty=0), **bad)
        with pytest.raises(rsdsfm.RsdsfmError):
            _clip_run(rsdsfm, torch, clip, 0, False, kw["radius"], kw["window_in"], one_call=True, margin=kw["margin"], max_empty=kw["max_empty"])


def test_evaluate_real_sequence_with_crop(rsdsfm, clip, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, fill=2, crop=True) and without fill: what it returned before, every frame as
    Solver.stabilize_cropped gives it through the window Solver.crop_window finds, and the files; without crop the keys and values of a call made
    without the new argument"""
    frames, rows, cols, K, gamma, seeds = clip
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, out_dir=str(tmp_path / "crop"), fill=2, crop=True, crop_margin=0, crop_max_empty=200, **kw)
        plain = ev(s, frames, out_dir=str(tmp_path / "plain"), fill=2, **kw)
        nofill = ev(s, frames, out_dir=str(tmp_path / "nofill"), crop=True, crop_margin=0, crop_max_empty=200, **kw)
        ps = out["path_smoothed"]
        maps, Rs, ts = [o["depth_map"] for o in out["pairs"]], [o["R"] for o in out["pairs"]], [o["t"] for o in out["pairs"]]
        window = s.crop_window([s.stabilize_filled(frames, maps, Rs, ts, K, out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], p, ps["M"][p], ps["m"][p], radius=2)[1]
                                for p in range(4)], 200, 0)
        again = [s.stabilize_cropped(frames, maps, Rs, ts, K, out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], p, ps["M"][p], ps["m"][p], window, radius=2)
                 for p in range(4)]
        window0 = s.crop_window(nofill["stab_masks"], 200, 0)
        again0 = [s.stabilize_cropped(frames, maps, Rs, ts, K, out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], p, ps["M"][p], ps["m"][p], window0, radius=0)
                  for p in range(4)]
        with pytest.raises(ValueError):
            ev(s, frames, camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, crop=True)
    new = {"stab_cropped", "crop_window", "crop_counts"}
    assert set(out) == set(plain) | new and set(nofill) == (set(plain) - {"stab_filled", "stab_sources", "fill_counts"}) | new
    assert out["crop_window"] == window and window[2] >= 1 and nofill["crop_window"] == window0 and window0[2] >= 1
    for name in ("scales", "A", "c", "broken", "stab_valid", "fill_counts"):
        assert np.array_equal(np.asarray(out[name]), np.asarray(plain[name])), name
    assert out["crop_counts"].shape == (4, 6) and nofill["crop_counts"].shape == (4, 2)
    for p in range(4):
        for k in ("stabilized", "stab_masks", "stab_filled", "stab_sources"):
            assert np.array_equal(out[k][p], plain[k][p]), (k, p)
        assert np.array_equal(out["stab_cropped"][p], again[p][0]) and out["crop_counts"][p].tolist() == again[p][3].tolist()
        assert np.array_equal(nofill["stab_cropped"][p], again0[p][0]) and nofill["crop_counts"][p].tolist() == again0[p][3].tolist()
        assert np.array_equal(rsdsfm.formats.read_png(str(tmp_path / "crop" / ("stabilized_cropped_%d.png" % p))), again[p][0])
    lines = (tmp_path / "crop" / "crop.csv").read_text().strip().split("\n")
    assert lines[0] == "window," + ",".join(str(x) for x in window) and lines[1] == "pair,none,own,prev1,next1,prev2,next2" and len(lines) == 6
    assert lines[2].split(",")[1:] == [str(x) for x in out["crop_counts"][0]]
    assert (tmp_path / "nofill" / "crop.csv").read_text().split("\n")[1] == "pair,none,own"
    assert sorted(x.name for x in (tmp_path / "plain").iterdir()) == sorted(x.name for x in (tmp_path / "crop").iterdir() if "crop" not in x.name)
