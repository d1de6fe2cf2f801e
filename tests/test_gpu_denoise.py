"""GPU: the temporal denoise (include/rsdsfm_denoise.h) bit for bit against its definition (tests/denoise_spec_numpy.py) in both library builds
-- the accumulate alone at the shapes where its 16 x 64 tile can go wrong, the cells after every step, the impulse's 3 x 3 footprint across
tile borders, the blend's record as a call of its own, the frame call on every case of tests/denoise_cases.py against the golden fixture the
CPU suite holds to the definition and against the public calls made one after another, the clip call against the frame calls, argument
errors.  Every plane has 16 guard bytes behind it, the outputs are never preset, the cells are preset to 0xFFFF, the inputs are verified
unchanged."""
import os

import numpy as np
import pytest

import denoise_cases as cases
import denoise_spec_numpy as spec
import stabilize_blend_spec_numpy as blend

pytestmark = pytest.mark.gpu

GUARD = 0xCD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_denoise_v1.npz")


def _guarded(torch, dev, a):
    """a's bytes on the device with 16 guard bytes behind them: (the view of a's shape, the guard)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + 16,), GUARD, dtype=torch.uint8, device=dev)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[:a.size].view(*a.shape), buf[a.size:]


def _outputs(torch, dev, image_shape, plane_shape):
    """the three output planes, never preset (every byte GUARD, and 16 guard bytes behind each), and the counters with a guard on either side"""
    planes = [_guarded(torch, dev, np.full(shape, GUARD, dtype=np.uint8)) for shape in (image_shape, plane_shape, plane_shape)]
    return planes, torch.full((5,), -1, dtype=torch.int64, device=dev)


def _collect(planes, cnt, guards=(), with_weight=True, with_counts=True):
    for g in [p[1] for p in planes] + list(guards):
        assert (g.cpu().numpy() == GUARD).all()
    c = cnt.cpu().numpy().tolist()
    assert c[0] == -1 and c[4] == -1 and (with_counts or c[1:4] == [-1] * 3)
    (d_img, _), (d_mask, _), (d_w, _) = planes
    weight = d_w.cpu().numpy()
    assert with_weight or (weight == GUARD).all()
    return dict(image=d_img.cpu().numpy(), mask=d_mask.cpu().numpy(), weight=weight, counts=c[1:4])


def _same(got, want, name="", weight=True, counts=True):
    for k in ("image", "mask") + (("weight",) if weight else ()):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert not counts or list(got["counts"]) == list(want["counts"]), (name, got["counts"], want["counts"])


def _cells(torch, dev, rows, cols, channels, value=0xFFFF):
    a = np.full((rows, cols, channels + 1), value, dtype=np.uint16)
    return _guarded(torch, dev, a.view(np.uint8))


def _cells_host(d_cells, rows, cols, channels):
    return d_cells.cpu().numpy().view(np.uint16).reshape(rows, cols, channels + 1)


def _record(torch, dev, rec):
    return None if rec is None else torch.from_numpy(np.ascontiguousarray(rec, dtype=np.uint64).view(np.int64)).to(dev)


def _denoise(torch, s, ref, rmask, layers, records=None, with_weight=True, with_counts=True, check_cells=True, **kw):
    """the layers through rsdsfm_denoise_accumulate_dev one after another on guarded planes, the cells preset to 0xFFFF and the outputs never
    preset; after every step that is not the last the cells are compared with the definition's, and the last launch must leave them as they
    were.  -> the collected outputs"""
    dev = torch.device("cuda", 0)
    rows, cols = rmask.shape
    ch = 1 if ref.ndim == 2 else 3
    L = len(layers)
    (d_ref, g_ref), (d_rm, g_rm) = _guarded(torch, dev, ref), _guarded(torch, dev, rmask)
    d_l = [(_guarded(torch, dev, i), _guarded(torch, dev, m)) for i, m in layers]
    d_rec = [_record(torch, dev, records[j] if records is not None else None) for j in range(L)]
    d_cells, cells_guard = _cells(torch, dev, rows, cols, ch)
    planes, cnt = _outputs(torch, dev, ref.shape, (rows, cols))
    torch.cuda.synchronize()
    outs = dict(d_image_out=planes[0][0].data_ptr(), d_mask_out=planes[1][0].data_ptr(), d_weight=planes[2][0].data_ptr() if with_weight else None,
                d_counts3=cnt[1:].data_ptr() if with_counts else None)
    if L == 0:
        s.denoise_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), None, None, ch, rows, cols, None, True, True, **outs, **kw)
    want_cells = np.full((rows, cols, ch + 1), 0xFFFF, dtype=np.uint16)
    for j, ((d_i, _), (d_m, _)) in enumerate(d_l):
        s.denoise_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_i.data_ptr(), d_m.data_ptr(), ch, rows, cols, d_cells.data_ptr(), j == 0, j == L - 1,
                                 d_sums8=d_rec[j].data_ptr() if d_rec[j] is not None else None, **outs, **kw)
        if j < L - 1:  # the last launch does not write the cells
            want_cells = spec.step(None if j == 0 else want_cells, ref, rmask, layers[j][0], layers[j][1], j == 0, records[j] if records is not None else None,
                                   kw.get("min_overlap", 0) or spec.MIN_OVERLAP_DEFAULT, kw.get("gain_mode", 0), kw.get("strength", 0) or spec.STRENGTH_DEFAULT)
        if check_cells or j >= L - 2:
            s.synchronize()
            assert np.array_equal(_cells_host(d_cells, rows, cols, ch), want_cells), ("cells after step", j, L)
    s.synchronize()
    assert np.array_equal(d_ref.cpu().numpy(), ref) and np.array_equal(d_rm.cpu().numpy(), rmask)  # the inputs are only read
    for ((d_i, _), (d_m, _)), (i, m) in zip(d_l, layers):
        assert np.array_equal(d_i.cpu().numpy(), i) and np.array_equal(d_m.cpu().numpy(), m)
    if L == 0:
        assert (d_cells.cpu().numpy() == 0xFF).all()
    guards = [g_ref, g_rm, cells_guard] + [g for (_, gi), (_, gm) in d_l for g in (gi, gm)]
    return _collect(planes, cnt, guards, with_weight, with_counts)


# ---------------------------------------------------------------------------------------------------
# the accumulate
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_accumulate_equals_the_definition(rsdsfm, arith, channels):
    """every shape -- one word, odd sizes, one under, exactly one and one over the tile in both directions, rows that start on every byte of a
    dword, 25 workgroups --, 1, 2 and 14 layers (first and last together, apart, and with mid steps between), no layer; masks with empty, full
    and mixed words and values other than 0 / 1, random bytes under unset mask bytes; records that drive each gain clamp, a plain gain, too
    small an overlap, and no record; the cells after every step; with and without the weight plane and the counters"""
    import torch

    seen = np.zeros(3, dtype=np.int64)
    rec = cases.records(channels)
    keys = ["plain", "low", "high", "small", "zero", None]
    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in cases.ACC_SHAPES:
            ref, rmask = cases.reference(*shape, channels)
            for L in cases.ACC_LAYERS:
                ls = cases.layers(ref, *shape, channels, L)
                recs = [rec[k] if k else None for k in (keys * 3)[:L]]
                strength = {1: 12, 2: 40, 14: 25}[L]
                got = _denoise(torch, s, ref, rmask, ls, recs, strength=strength, check_cells=L <= 2 or shape in ((17, 65), (37, 67)))
                want = spec.denoise(ref, rmask, ls, recs, strength=strength)
                _same(got, want, (shape, L))
                seen += np.array(want["counts"])
            _same(_denoise(torch, s, ref, rmask, []), spec.denoise(ref, rmask, []), (shape, 0))
            ls = cases.layers(ref, *shape, channels, 2, seed=1)
            want = spec.denoise(ref, rmask, ls, None, gain_mode=1, min_overlap=7)
            for with_weight, with_counts in ((False, True), (True, False), (False, False)):
                _same(_denoise(torch, s, ref, rmask, ls, None, with_weight, with_counts, gain_mode=1, min_overlap=7), want, shape, with_weight, with_counts)
        assert rsdsfm.denoise_accumulate_launches() == 1
    assert (seen > 0).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_every_gain_and_the_largest_sums(rsdsfm, channels):
    """one layer per record of denoise_cases.records with and without gain_mode 1 and with a min_overlap above the record's count; fourteen
    layers of 255 on a reference of 255: n = 240, s = 61 200 in every cell"""
    import torch

    with rsdsfm.Solver(0) as s:
        ref, rmask = cases.reference(33, 129, channels, seed=2)
        ls = cases.layers(ref, 33, 129, channels, 1, seed=2)
        for key, r in cases.records(channels).items():
            for kw in (dict(), dict(gain_mode=1), dict(min_overlap=6000)):
                _same(_denoise(torch, s, ref, rmask, ls, [r], strength=60, **kw), spec.denoise(ref, rmask, ls, [r], strength=60, **kw), (key, kw))
        shape = (17, 65) if channels == 1 else (17, 65, 3)
        sat, full = np.full(shape, 255, dtype=np.uint8), np.full((17, 65), 200, dtype=np.uint8)
        got = _denoise(torch, s, sat, full, [(sat, full)] * 14, check_cells=False)
        assert (got["image"] == 255).all() and (got["weight"] == 240).all() and got["counts"] == [0, 0, 17 * 65]


@pytest.mark.parametrize("channels", [1, 3])
def test_the_impulse_shows_the_3x3_footprint_across_tile_borders(rsdsfm, channels):
    """reference and layer equal but for one pixel, at every corner and edge midpoint of every tile and of the frame: with h = 1 the weight plane
    is 16 on the 3 x 3 window about the pixel (inside the frame) and 32 everywhere else -- the definition's, across the tile's borders"""
    import torch

    with rsdsfm.Solver(0) as s:
        for rows, cols in ((33, 129), (17, 65)):
            ref, _ = cases.reference(rows, cols, channels, seed=3)
            full = np.ones((rows, cols), dtype=np.uint8)
            positions = cases.impulse_positions(rows, cols)
            assert {(0, 0), (rows - 1, cols - 1), (15, 63), (16, 64), (15, 64), (16, 63), (8, 64), (16, 32)} <= set(positions)
            for y, x in positions:
                layer = ref.copy()
                layer[y, x] = layer[y, x] ^ 0x40  # |d| = 64 in every channel
                got = _denoise(torch, s, ref, full, [(layer, full)], strength=1, with_counts=False, check_cells=False)
                want = np.full((rows, cols), 32, dtype=np.uint8)
                want[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 16
                assert np.array_equal(got["weight"], want), (rows, cols, y, x)
                _same(got, spec.denoise(ref, full, [(layer, full)], strength=1), (y, x), counts=False)


def test_the_host_convenience_of_the_accumulate(rsdsfm):
    ref, rmask = cases.reference(37, 67, 3)
    ls = cases.layers(ref, 37, 67, 3, 3)
    recs = [cases.records(3)["plain"], None, cases.records(3)["low"]]
    with rsdsfm.Solver(0) as s:
        img, mask, w, counts = s.denoise_accumulate(ref, rmask, ls, recs, strength=30)
        _same(dict(image=img, mask=mask, weight=w, counts=counts.tolist()), spec.denoise(ref, rmask, ls, recs, strength=30))
        img, mask, w, counts = s.denoise_accumulate(ref, rmask, [])
        _same(dict(image=img, mask=mask, weight=w, counts=counts.tolist()), spec.denoise(ref, rmask, []))


@pytest.mark.parametrize("channels", [1, 3])
def test_the_overlap_sums_call_equals_the_blends_record(rsdsfm, channels):
    import torch

    dev = torch.device("cuda", 0)
    with rsdsfm.Solver(0) as s:
        for shape in ((2, 2), (5, 5), (37, 67), (70, 300)):
            ref, rmask = cases.reference(*shape, channels, seed=4)
            (layer, lmask), = cases.layers(ref, *shape, channels, 1, seed=4)
            source = np.where(rmask != 0, np.random.default_rng(shape[1]).choice(np.array([1, 1, 1, 2, 5]), size=shape), 0).astype(np.uint8)
            planes = [_guarded(torch, dev, a) for a in (ref, source, layer, lmask)]
            d_rec = torch.full((10,), -1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            s.seam_overlap_sums_dev(planes[0][0].data_ptr(), planes[1][0].data_ptr(), planes[2][0].data_ptr(), planes[3][0].data_ptr(), channels, *shape, d_rec[1:].data_ptr())
            s.synchronize()
            got = d_rec.cpu().numpy()
            assert got[0] == -1 and got[9] == -1 and np.array_equal(got[1:9].view(np.uint64), blend.overlap_sums(ref, source, layer, lmask)), shape
            for (d, g), a in zip(planes, (ref, source, layer, lmask)):
                assert np.array_equal(d.cpu().numpy(), a) and (g.cpu().numpy() == GUARD).all()
        a = torch.zeros(64, dtype=torch.uint8, device=dev)
        for bad in (dict(i=0), dict(l=0), dict(rec=0), dict(i=a.data_ptr() + 1), dict(rec=d_rec.data_ptr() + 4), dict(ch=2), dict(r=1), dict(c=16385)):
            kw = dict(dict(i=a.data_ptr(), src=a.data_ptr(), l=a.data_ptr(), m=a.data_ptr(), ch=1, r=8, c=8, rec=d_rec[1:].data_ptr()), **bad)
            with pytest.raises(rsdsfm.RsdsfmError):
                s.seam_overlap_sums_dev(kw["i"], kw["src"], kw["l"], kw["m"], kw["ch"], kw["r"], kw["c"], kw["rec"])
        s.synchronize()
        assert np.array_equal(d_rec.cpu().numpy(), got)  # nothing was enqueued


def test_accumulate_argument_errors(rsdsfm):
    """every refusal returns RSDSFM_ERR_INVALID and enqueues nothing: the outputs and the cells keep their sentinel; after a refused call the
    same call without the fault goes through"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    u8 = lambda value, *shape: torch.full(shape, value, dtype=torch.uint8, device=dev)
    ref, rmask, lay, lmask = u8(9, rows, cols, 3), u8(1, rows, cols), u8(9, rows, cols, 3), u8(1, rows, cols)
    out, omask, wplane = u8(GUARD, rows, cols + 4, 3), u8(GUARD, rows, cols + 4), u8(GUARD, rows, cols + 4)
    cells = torch.full((rows, cols + 4, 4), 0x7BCD, dtype=torch.int16, device=dev)
    counts = torch.full((5,), -1, dtype=torch.int64, device=dev)
    rec = torch.zeros(9, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        def acc(R=ref.data_ptr(), mR=rmask.data_ptr(), L=lay.data_ptr(), mL=lmask.data_ptr(), ch=3, r=rows, c=cols, cl=cells.data_ptr(), first=1, last=1, rc=rec.data_ptr(),
                mo=0, gm=0, h=12, o=out.data_ptr(), k=omask.data_ptr(), wp=wplane.data_ptr(), cnt=counts[1:].data_ptr()):
            return s.denoise_accumulate_dev(R, mR, L, mL, ch, r, c, cl, first, last, rc, mo, gm, h, o, k, wp, cnt)

        bads = (dict(R=0), dict(mR=0), dict(L=0), dict(mL=0), dict(L=0, mL=0, first=0), dict(L=0, mL=0, last=0), dict(o=0), dict(k=0), dict(cl=0, first=0), dict(cl=0, last=0),
                dict(R=ref.data_ptr() + 1), dict(mR=rmask.data_ptr() + 2), dict(L=lay.data_ptr() + 3), dict(mL=lmask.data_ptr() + 1), dict(o=out.data_ptr() + 1),
                dict(k=omask.data_ptr() + 2), dict(wp=wplane.data_ptr() + 3), dict(cl=cells.data_ptr() + 4), dict(cnt=counts.data_ptr() + 4), dict(rc=rec.data_ptr() + 4),
                dict(o=ref.data_ptr()), dict(k=rmask.data_ptr()), dict(wp=lay.data_ptr()), dict(o=lmask.data_ptr()), dict(o=cells.data_ptr()), dict(k=out.data_ptr()),
                dict(wp=omask.data_ptr()), dict(wp=out.data_ptr()), dict(cl=ref.data_ptr()), dict(cl=lmask.data_ptr()), dict(mR=ref.data_ptr()), dict(L=ref.data_ptr()),
                dict(mL=lay.data_ptr()), dict(ch=2), dict(ch=4), dict(r=1), dict(c=16385), dict(r=16385), dict(c=1), dict(first=2), dict(last=-1), dict(h=-1), dict(h=256),
                dict(gm=2), dict(gm=-1), dict(mo=-1))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                acc(**bad)
        s.synchronize()
        for x in (out, omask, wplane):  # nothing was enqueued
            assert (x.cpu().numpy() == GUARD).all()
        assert (cells.cpu().numpy().view(np.uint16) == 0x7BCD).all() and counts.cpu().numpy().tolist() == [-1] * 5
        for bad in bads[:3]:
            with pytest.raises(rsdsfm.RsdsfmError):
                acc(**bad)
            acc()  # the same call without the fault goes through
        acc(cl=0, wp=None, cnt=None)  # first and last: the cells may be NULL
        s.synchronize()
        flat = out.cpu().numpy().reshape(-1)
        assert (flat[:rows * cols * 3] == 9).all() and (flat[rows * cols * 3:] == GUARD).all() and (omask.cpu().numpy().reshape(-1)[:rows * cols] == 1).all()
        assert counts.cpu().numpy().tolist() == [-1, 0, 0, rows * cols, -1] and (wplane.cpu().numpy().reshape(-1)[:rows * cols] == 32).all()
        # not last: the outputs are not read -- NULL and misaligned ones pass, and nothing is written to them
        acc(last=0, o=0, k=0, wp=0, cnt=0)
        acc(last=0, first=0, o=out.data_ptr() + 1, k=3, wp=5, cnt=counts.data_ptr() + 4)
        s.synchronize()
        c16 = cells.cpu().numpy().view(np.uint16).reshape(-1)[:rows * cols * 4].reshape(-1, 4)
        assert (c16 == [48 * 9, 48 * 9, 48 * 9, 48]).all() and counts.cpu().numpy().tolist() == [-1, 0, 0, rows * cols, -1]
        assert (cells.cpu().numpy().view(np.uint16).reshape(-1)[rows * cols * 4:] == 0x7BCD).all()


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
def _clip(torch, dev, case):
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(frames=[tt(x) for x in case["frames"]], maps=[tt(z.T) for z in case["depths"]], Rs=[tt(np.asarray(R).reshape(-1, 9)) for R in case["Rs"]],
                ts=[tt(t) for t in case["ts"]])


def _frame_kw(case):
    return dict(strength=case["strength"], gain=case["gain_mode"] == 0, min_overlap=case["min_overlap"], window=case["window"], occlusion=case["occlusion"],
                occlusion_tol_q16=case["tol_q16"], mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])


def _frame(torch, s, case, d=None, q=None, with_weight=True, with_counts=True):
    """one rsdsfm_denoise_frame_dev of frame q of a case (the context's knob set to the case's) into guarded, never preset outputs"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = d or _clip(torch, dev, case)
    src, M, m = cases.sources_and_poses(case, q)
    planes, cnt = _outputs(torch, dev, case["frames"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    s.set_occlusion_search(case["search"])
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    s.denoise_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, planes[0][0].data_ptr(), planes[1][0].data_ptr(),
                        planes[2][0].data_ptr() if with_weight else None, cnt[1:].data_ptr() if with_counts else None, **_frame_kw(case))
    s.synchronize()
    s.set_occlusion_search(0)
    for k, key in (("frames", "frames"),):
        for t, a in zip(d[k], case[key]):
            assert np.array_equal(t.cpu().numpy(), a)
    return _collect(planes, cnt, (), with_weight, with_counts)


def _parts(torch, s, case):
    """the public calls one after another on planes of the test's own: the own frame's window render (id 1, with a source plane) onto zeroed
    planes, then per neighbour the render alone onto a zeroed layer, rsdsfm_seam_overlap_sums_dev and rsdsfm_denoise_accumulate_dev"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = _clip(torch, dev, case)
    src, M, m = cases.sources_and_poses(case)
    z = lambda like=None: torch.zeros_like(d["frames"][0]) if like is None else torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
    d_ref, d_rm, d_rs = z(), z(1), z(1)
    d_cells = torch.full((rows, cols, ch + 1), -1, dtype=torch.int16, device=dev)
    d_rec = torch.full((8,), -1, dtype=torch.int64, device=dev)
    planes, cnt = _outputs(torch, dev, case["frames"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    kw = dict(mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    arg = lambda k: (d["frames"][src[k]].data_ptr(), ch, d["maps"][src[k]].data_ptr(), d["Rs"][src[k]].data_ptr(), d["ts"][src[k]].data_ptr(), case["K"], rows, cols, M[k], m[k])
    s.stabilize_window_frame_dev(*arg(0), 1, case["window"], d_ref.data_ptr(), d_rm.data_ptr(), d_rs.data_ptr(), **kw)
    outs = dict(d_image_out=planes[0][0].data_ptr(), d_mask_out=planes[1][0].data_ptr(), d_weight=planes[2][0].data_ptr(), d_counts3=cnt[1:].data_ptr())
    acc = dict(min_overlap=case["min_overlap"], gain_mode=case["gain_mode"], strength=case["strength"])
    if len(src) == 1:
        s.denoise_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), None, None, ch, rows, cols, None, True, True, **acc, **outs)
    for k in range(1, len(src)):
        d_l, d_lm = z(), z(1)
        torch.cuda.synchronize()
        if case["occlusion"] and case["search"]:
            s.stabilize_search_frame_dev(*arg(k), 2, case["window"], d_l.data_ptr(), d_lm.data_ptr(), tol_q16=case["tol_q16"], **kw)
        elif case["occlusion"]:
            s.stabilize_visible_frame_dev(*arg(k), 2, case["window"], d_l.data_ptr(), d_lm.data_ptr(), tol_q16=case["tol_q16"], **kw)
        else:
            s.stabilize_window_frame_dev(*arg(k), 2, case["window"], d_l.data_ptr(), d_lm.data_ptr(), **kw)
        s.seam_overlap_sums_dev(d_ref.data_ptr(), d_rs.data_ptr(), d_l.data_ptr(), d_lm.data_ptr(), ch, rows, cols, d_rec.data_ptr())
        s.denoise_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_l.data_ptr(), d_lm.data_ptr(), ch, rows, cols, d_cells.data_ptr(), k == 1, k == len(src) - 1,
                                 d_sums8=d_rec.data_ptr(), **acc, **outs)
        s.synchronize()  # d_l and d_lm are released at the end of the iteration
    s.synchronize()
    return _collect(planes, cnt), dict(image=d_ref.cpu().numpy(), mask=d_rm.cpu().numpy())


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_every_case_equals_the_definition_and_the_public_calls(oracle, rsdsfm, arith):
    """image, mask, weight plane and the three counts of every fixture case -- the noisy shift scene, a fold pair plain, through the occlusion
    test and through the search, a zoomed window, gained neighbours with the gain on, off and under too small an overlap, five sources from
    the clip's middle and one-sided from its ends, one source, the 2 x 2 dense case -- against the golden fixture, and against the public
    calls made one after another; one source alone is the window render"""
    import torch

    g = np.load(GOLDEN)
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in cases.all_cases(oracle.pose_table):
            n = case["name"] + "/"
            want = dict(image=g[n + "image"], mask=g[n + "mask"], weight=g[n + "weight"], counts=g[n + "counts"].tolist())
            _same(_frame(torch, s, case), want, n)
            s.set_occlusion_search(case["search"])
            parts, ref = _parts(torch, s, case)
            s.set_occlusion_search(0)
            _same(parts, want, n + " parts")
            if len(cases.sources_and_poses(case)[0]) == 1:
                assert np.array_equal(want["image"], ref["image"]) and np.array_equal(want["mask"], ref["mask"])
            rows, cols = case["depths"][0].shape
            nsrc = len(cases.sources_and_poses(case)[0])
            assert rsdsfm.denoise_launches(rows, cols, nsrc) == nsrc * rsdsfm.stabilize_window_launches(rows, cols) + (1 if nsrc == 1 else 2 * (nsrc - 1))
        case = cases.all_cases(oracle.pose_table)[0]
        want = cases.run_spec(case)
        for with_weight, with_counts in ((False, True), (True, False)):
            _same(_frame(torch, s, case, with_weight=with_weight, with_counts=with_counts), want, "optional outputs", with_weight, with_counts)


def test_frame_argument_errors(oracle, rsdsfm):
    """a refused frame call enqueues nothing: the outputs keep their guard bytes"""
    import torch

    dev = torch.device("cuda", 0)
    case = [c for c in cases.all_cases(oracle.pose_table) if c["name"] == "gained"][0]
    rows, cols = case["depths"][0].shape
    d = _clip(torch, dev, case)
    src, M, m = cases.sources_and_poses(case)
    planes, cnt = _outputs(torch, dev, case["frames"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    with rsdsfm.Solver(0) as s:
        def call(images=pick("frames"), maps=pick("maps"), M=M, m=m, o=planes[0][0].data_ptr(), k=planes[1][0].data_ptr(), w=planes[2][0].data_ptr(),
                 cnt_=cnt[1:].data_ptr(), ch=3, **kw):
            return s.denoise_frame_dev(images, ch, maps, pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, o, k, w, cnt_, **kw)

        bad_M = M.copy()
        bad_M[1, 0, 0] = np.nan
        params = rsdsfm.DenoiseParams()
        params.struct_bytes = 40
        bads = (dict(images=[0] + pick("frames")[1:]), dict(maps=pick("maps")[:2] + [0]), dict(images=[]), dict(images=pick("frames") * 6, maps=pick("maps") * 6, M=np.tile(M, (6, 1, 1)), m=np.tile(m, (6, 1))),
                dict(M=bad_M), dict(o=0), dict(k=0), dict(o=planes[1][0].data_ptr()), dict(w=planes[0][0].data_ptr()), dict(o=planes[0][0].data_ptr() + 1),
                dict(cnt_=cnt.data_ptr() + 4), dict(o=pick("frames")[2]), dict(ch=2), dict(strength=256), dict(strength=-1), dict(min_overlap=-1), dict(occlusion=2),
                dict(occlusion=True, occlusion_tol_q16=65537), dict(window=(0, 0, rows + 1, cols)), dict(window=(1, 1, 0, 4)), dict(iterations=17), dict(params=params))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        for (p, gd) in planes:
            assert (p.cpu().numpy() == GUARD).all() and (gd.cpu().numpy() == GUARD).all()
        assert cnt.cpu().numpy().tolist() == [-1] * 5
        call(strength=case["strength"])
        s.synchronize()
        _same(_collect(planes, cnt), cases.run_spec(case))


# ---------------------------------------------------------------------------------------------------
# the clip call
# ---------------------------------------------------------------------------------------------------
def _video(torch, s, case, want_counts=True, with_weights=True):
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    ns = len(case["depths"])
    d = _clip(torch, dev, case)
    outs = [_outputs(torch, dev, case["frames"][0].shape, (rows, cols)) for _ in range(ns)]
    torch.cuda.synchronize()
    ptrs = lambda a: [x.data_ptr() for x in a]
    kw = _frame_kw(case)
    s.set_occlusion_search(case["search"])
    r = s.denoise_video_dev(ptrs(d["frames"]), rows, cols, ch, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"], case["c_path"],
                            case["scales"], [p[0][0].data_ptr() for p, _ in outs], [p[1][0].data_ptr() for p, _ in outs],
                            [p[2][0].data_ptr() for p, _ in outs] if with_weights else None, want_counts=want_counts, radius=case["radius"], **kw)
    s.synchronize()
    s.set_occlusion_search(0)
    got = []
    for q, (planes, cnt) in enumerate(outs):
        one = _collect(planes, cnt, (), with_weights, False)
        one["counts"] = r["counts"][q].tolist() if want_counts else None
        got.append(one)
    return got, d


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_clip_call_equals_the_frame_calls(oracle, rsdsfm, arith):
    """three sources (radius 1) and five (radius 2, the first and last frames with one-sided neighbours; the noisy shift scene, whose path is the
    chain itself, and a smooth clip on a path of its own) and one source alone: every frame of the clip call is the frame call's, which is the
    definition's; without the counters and the weight planes the call only enqueues"""
    import torch

    every = {c["name"]: c for c in cases.all_cases(oracle.pose_table)}
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in (every["gained"], every["five-middle"], every["shift-bgr-0"], every["one-source"], dict(every["fold-search"], radius=2)):
            got, d = _video(torch, s, case)
            ns = len(case["depths"])
            for q in range(ns):
                want = cases.run_spec(case, q)
                _same(got[q], want, (case["name"], q))
                _same(_frame(torch, s, case, d, q), want, (case["name"], q, "frame"))
            if ns == 5:
                assert [len(cases.sources_and_poses(case, q)[0]) for q in range(5)] == [3, 4, 5, 4, 3]
        case = every["five-middle"]
        got, _ = _video(torch, s, case, want_counts=False, with_weights=False)
        for q in range(5):
            _same(got[q], cases.run_spec(case, q), q, weight=False, counts=False)
        # a refused clip call enqueues nothing
        dev = torch.device("cuda", 0)
        rows, cols = case["depths"][0].shape
        d = _clip(torch, dev, case)
        outs = [_outputs(torch, dev, case["frames"][0].shape, (rows, cols)) for _ in range(5)]
        torch.cuda.synchronize()
        ptrs = lambda a: [x.data_ptr() for x in a]
        bad_scales = case["scales"].copy()
        bad_scales[4] = 0.0

        def call(scales=case["scales"], o=None, **kw):
            return s.denoise_video_dev(ptrs(d["frames"]), rows, cols, 1, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"],
                                       case["c_path"], scales, o or [p[0][0].data_ptr() for p, _ in outs], [p[1][0].data_ptr() for p, _ in outs], None, **kw)

        for bad in (dict(scales=bad_scales), dict(radius=8), dict(radius=-1), dict(strength=300), dict(o=[outs[0][0][0][0].data_ptr()] * 4 + [0]),
                    dict(o=[outs[0][0][0][0].data_ptr()] * 4 + [d["frames"][1].data_ptr()])):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        for planes, _ in outs:
            for p, gd in planes:
                assert (p.cpu().numpy() == GUARD).all() and (gd.cpu().numpy() == GUARD).all()


# ---------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------
def test_evaluate_real_sequence_with_denoise(rsdsfm, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, denoise=K or (K, strength)) adds exactly stab_denoised, denoise_masks, denoise_weights and
    denoise_counts and the files stabilized_denoised_<p>.png and denoise.csv, and frame 0 is the frame call's on the clip's own outputs; without
    the keyword every key and file is what it was"""
    import torch

    from test_gpu_stabilize_search import TRIALS, plain_clip

    frames, rows, cols, K, gamma, seeds, _ = plain_clip(rsdsfm)
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
    n = len(frames) - 1
    dev = torch.device("cuda", 0)
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, denoise=(1, 30), out_dir=str(tmp_path / "with"), **kw)
        plain = ev(s, frames, out_dir=str(tmp_path / "without"), **kw)
        default = ev(s, frames, denoise=2, **kw)
        ps, o = out["path_smoothed"], out["pairs"]
        src, _, M0, m0, _, _ = rsdsfm.retime_poses(out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], 0.0, nsources=n)
        nb, _, Mn, mn = rsdsfm.neighbour_poses(out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], 0, 1)
        order = list(src) + list(nb)
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_f, d_z = [tt(frames[q]) for q in order], [tt(np.asarray(o[q]["depth_map"]).T) for q in order]
        d_R, d_t = [tt(np.asarray(o[q]["R"]).reshape(-1, 9)) for q in order], [tt(o[q]["t"]) for q in order]
        planes, cnt = _outputs(torch, dev, frames[0].shape, (rows, cols))
        torch.cuda.synchronize()
        ptrs = lambda a: [x.data_ptr() for x in a]
        s.denoise_frame_dev(ptrs(d_f), 3, ptrs(d_z), ptrs(d_R), ptrs(d_t), K, rows, cols, np.concatenate([M0, Mn]), np.concatenate([m0, mn]), planes[0][0].data_ptr(),
                            planes[1][0].data_ptr(), planes[2][0].data_ptr(), cnt[1:].data_ptr(), strength=30)
        s.synchronize()
        one = _collect(planes, cnt)
    new = {"stab_denoised", "denoise_masks", "denoise_weights", "denoise_counts"}
    assert set(out) == set(plain) | new == set(default)
    assert len(out["stab_denoised"]) == len(out["denoise_masks"]) == len(out["denoise_weights"]) == n and out["denoise_counts"].shape == (n, 3)
    _same(dict(image=out["stab_denoised"][0], mask=out["denoise_masks"][0], weight=out["denoise_weights"][0], counts=out["denoise_counts"][0].tolist()), one)
    for p in range(n):
        assert out["stab_denoised"][p].shape == frames[0].shape and out["denoise_counts"][p].sum() == rows * cols
        assert np.array_equal(out["denoise_masks"][p], (out["denoise_weights"][p] > 0).astype(np.uint8))  # set where anything counted
        assert out["denoise_weights"][p].max() <= 32 and default["denoise_weights"][p].max() <= 16 * n
    assert sum(int(c[2]) for c in out["denoise_counts"]) > 0  # something was averaged
    for k in plain:
        if k not in ("pairs", "path_smoothed", "links"):
            assert np.asarray(out[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    with_files, without_files = set(os.listdir(str(tmp_path / "with"))), set(os.listdir(str(tmp_path / "without")))
    assert with_files == without_files | {"stabilized_denoised_%d.png" % p for p in range(n)} | {"denoise.csv"}
    lines = open(str(tmp_path / "with" / "denoise.csv")).read().split()
    assert lines[0] == "pair,unset,own_only,averaged,mean_weight" and len(lines) == 1 + n
    assert lines[1].split(",")[:4] == ["0"] + [str(int(x)) for x in out["denoise_counts"][0]]
