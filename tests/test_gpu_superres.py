"""GPU: the multi-frame super-resolution (include/rsdsfm_superres.h) bit for bit against its definition (tests/superres_spec_numpy.py) in both
library builds -- the render alone at the shapes and scales where its groups of 4 fine pixels can go wrong, through a zoomed window, of a
source without a valid depth and of one with a non-identity pose and holes; the accumulate alone at the denoise's shapes, the cells after every
step, the impulse's 3 x 3 footprint across tile borders, every gain clamp; the frame call on every case of tests/superres_cases.py against the
golden fixture the CPU suite holds to the definition and against the public calls made one after another; the clip call against the frame
calls; argument errors; the evaluation's keyword.  Every plane has 16 guard bytes behind it, the outputs are never preset, the cells are
preset to 0xFFFF, the inputs are verified unchanged."""
import os

import numpy as np
import pytest

import superres_cases as cases
import superres_spec_numpy as spec

pytestmark = pytest.mark.gpu

GUARD = 0xCD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_superres_v1.npz")


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


def _fine(case):
    rows, cols = case["depths"][0].shape
    return case["scale"] * rows, case["scale"] * cols


def _fine_image_shape(case):
    return _fine(case) + tuple(case["frames"][0].shape[2:])


# ---------------------------------------------------------------------------------------------------
# the render
# ---------------------------------------------------------------------------------------------------
def _render(torch, s, src, scale, window=None, with_valid=True, iterations=0):
    """one rsdsfm_superres_render_dev into guarded, never preset planes -> dict(bil, near, prox, valid)"""
    dev = torch.device("cuda", 0)
    image = src["image"]
    rows, cols = image.shape[:2]
    ch = 1 if image.ndim == 2 else 3
    fine = (scale * rows, scale * cols)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    (d_i, g_i) = _guarded(torch, dev, image)
    d_z, d_R, d_t = tt(np.asarray(src["depth"], dtype=np.float64).T), tt(np.asarray(src["R"], dtype=np.float64).reshape(-1, 9)), tt(np.asarray(src["t"], dtype=np.float64))
    outs = [_guarded(torch, dev, np.full(shape, GUARD, dtype=np.uint8)) for shape in (fine + image.shape[2:], fine + image.shape[2:], fine, fine)]
    torch.cuda.synchronize()
    s.superres_render_dev(d_i.data_ptr(), ch, d_z.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), src["K"], rows, cols, src["M"], src["m"], scale, outs[0][0].data_ptr(),
                          outs[1][0].data_ptr(), outs[2][0].data_ptr(), outs[3][0].data_ptr() if with_valid else None, window, iterations=iterations)
    s.synchronize()
    assert np.array_equal(d_i.cpu().numpy(), image) and (g_i.cpu().numpy() == GUARD).all()
    for _, g in outs:
        assert (g.cpu().numpy() == GUARD).all()
    got = dict(bil=outs[0][0].cpu().numpy(), near=outs[1][0].cpu().numpy(), prox=outs[2][0].cpu().numpy(), valid=outs[3][0].cpu().numpy())
    assert with_valid or (got["valid"] == GUARD).all()
    return got


def _same_render(got, want, name, with_valid=True):
    for k in ("bil", "near", "prox"):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert not with_valid or np.array_equal(got["valid"], (want["prox"] != 0).astype(np.uint8)), (name, "valid")


@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_render_equals_the_definition(rsdsfm, arith, channels):
    """every shape and scale of superres_cases.RENDER_SHAPES -- one word at every scale, fine rows with a tail of 2, fine 18 x 66 across a tile both
    ways, scale 1 with a tail, scale 3 and 4 --, each as a pure upscale and with a non-identity pose and holes in the depth; a zoomed window; a
    source without a valid depth; with and without the validity plane; another iteration count"""
    import torch

    seen = set()
    with rsdsfm.Solver(0, arith=arith) as s:
        for rows, cols, scale in cases.RENDER_SHAPES:
            for kind in ("identity", "pose"):
                src = cases.render_source(rows, cols, channels, kind)
                want = spec.render(src["image"], src["depth"], src["R"], src["t"], src["K"], src["M"], src["m"], scale)
                _same_render(_render(torch, s, src, scale), want, (rows, cols, scale, kind))
                seen |= set(np.unique(want["prox"]).tolist())
            assert rsdsfm.superres_render_launches(rows, cols, scale) == rsdsfm.stabilize_window_launches(rows, cols)
        src = cases.render_source(9, 33, channels, "pose", seed=1)
        window = (1, 4, 6, (6 * 33) // 9)
        for scale in (1, 2, 3):
            want = spec.render(src["image"], src["depth"], src["R"], src["t"], src["K"], src["M"], src["m"], scale, window)
            _same_render(_render(torch, s, src, scale, window, with_valid=False), want, ("zoom", scale), with_valid=False)
        want = spec.render(src["image"], src["depth"], src["R"], src["t"], src["K"], src["M"], src["m"], 2, iterations=1)
        _same_render(_render(torch, s, src, 2, iterations=1), want, "one iteration")
        empty = cases.render_source(8, 22, channels, "empty")
        got = _render(torch, s, empty, 3)
        assert not got["bil"].any() and not got["near"].any() and not got["prox"].any() and not got["valid"].any()
    assert seen >= {0, 1, 4, 16}


@pytest.mark.parametrize("channels", [1, 3])
def test_scale_1_equals_the_window_frame_call(rsdsfm, channels):
    """at scale 1 bil and prox != 0 are byte for byte rsdsfm_stabilize_window_frame_dev's image and mask on zeroed planes, full and zoomed window"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 17, 65
    src = cases.render_source(rows, cols, channels, "pose", seed=2)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with rsdsfm.Solver(0) as s:
        for window in ((0, 0, rows, cols), (3, 5, 9, (9 * cols) // rows)):
            got = _render(torch, s, src, 1, window)
            d_i, d_z, d_R, d_t = tt(src["image"]), tt(src["depth"].T), tt(src["R"].reshape(-1, 9)), tt(src["t"])
            d_o, d_m = torch.zeros_like(d_i), torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            s.stabilize_window_frame_dev(d_i.data_ptr(), channels, d_z.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), src["K"], rows, cols, src["M"], src["m"], 1, window,
                                         d_o.data_ptr(), d_m.data_ptr())
            s.synchronize()
            assert np.array_equal(got["bil"], d_o.cpu().numpy()) and np.array_equal(got["valid"], d_m.cpu().numpy()) and d_m.any(), window


def test_render_argument_errors(rsdsfm):
    """every refusal returns RSDSFM_ERR_INVALID and enqueues nothing: the outputs keep their sentinel; the same call without the fault goes through"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols, scale = 8, 22, 2
    src = cases.render_source(rows, cols, 3, "pose")
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_i, d_z, d_R, d_t = tt(src["image"]), tt(src["depth"].T), tt(src["R"].reshape(-1, 9)), tt(src["t"])
    u8 = lambda *shape: torch.full(shape, GUARD, dtype=torch.uint8, device=dev)
    bil, near, prox, valid = u8(16, 44 + 4, 3), u8(16, 44 + 4, 3), u8(16, 44 + 4), u8(16, 44 + 4)
    torch.cuda.synchronize()
    bad_M = np.array(src["M"], dtype=np.float64)
    bad_M[0, 0] = np.inf
    with rsdsfm.Solver(0) as s:
        def call(i=d_i.data_ptr(), z=d_z.data_ptr(), ch=3, r=rows, c=cols, M=src["M"], m=src["m"], S=scale, b=bil.data_ptr(), n=near.data_ptr(), q=prox.data_ptr(),
                 v=valid.data_ptr(), **kw):
            return s.superres_render_dev(i, ch, z, d_R.data_ptr(), d_t.data_ptr(), src["K"], r, c, M, m, S, b, n, q, v, **kw)

        bads = (dict(i=0), dict(z=0), dict(b=0), dict(n=0), dict(q=0), dict(i=d_i.data_ptr() + 1), dict(b=bil.data_ptr() + 2), dict(n=near.data_ptr() + 1),
                dict(q=prox.data_ptr() + 3), dict(v=valid.data_ptr() + 1), dict(b=near.data_ptr()), dict(q=bil.data_ptr()), dict(v=prox.data_ptr()), dict(b=d_i.data_ptr()),
                dict(ch=2), dict(r=1), dict(c=16385), dict(S=0), dict(S=5), dict(S=-1), dict(r=8193, S=2), dict(c=4097, S=4), dict(M=bad_M),
                dict(m=[0.0, np.nan, 0.0]), dict(window=(0, 0, rows + 1, cols)), dict(window=(1, 1, 0, 4)), dict(window=(0, 20, 4, 4)), dict(iterations=17),
                dict(iterations=-1), dict(mode=7), dict(q5_mode=9))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        for x in (bil, near, prox, valid):  # nothing was enqueued
            assert (x.cpu().numpy() == GUARD).all()
        call()
        s.synchronize()
        want = spec.render(src["image"], src["depth"], src["R"], src["t"], src["K"], src["M"], src["m"], scale)
        n = 16 * 44
        assert np.array_equal(prox.cpu().numpy().reshape(-1)[:n].reshape(16, 44), want["prox"]) and (prox.cpu().numpy().reshape(-1)[n:] == GUARD).all()
        assert np.array_equal(bil.cpu().numpy().reshape(-1)[:3 * n].reshape(16, 44, 3), want["bil"]) and (bil.cpu().numpy().reshape(-1)[3 * n:] == GUARD).all()


def test_the_host_convenience_of_the_render(rsdsfm):
    src = cases.render_source(9, 33, 3, "pose")
    with rsdsfm.Solver(0) as s:
        got = s.superres_render(src["image"], src["depth"], src["R"], src["t"], src["K"], src["M"], src["m"], 2)
    _same_render(got, spec.render(src["image"], src["depth"], src["R"], src["t"], src["K"], src["M"], src["m"], 2), "host")


# ---------------------------------------------------------------------------------------------------
# the accumulate
# ---------------------------------------------------------------------------------------------------
def _cells(torch, dev, rows, cols, channels, value=0xFFFF):
    a = np.full((rows, cols, channels + 1), value, dtype=np.uint16)
    return _guarded(torch, dev, a.view(np.uint8))


def _cells_host(d_cells, rows, cols, channels):
    return d_cells.cpu().numpy().view(np.uint16).reshape(rows, cols, channels + 1)


def _record(torch, dev, rec):
    return None if rec is None else torch.from_numpy(np.ascontiguousarray(rec, dtype=np.uint64).view(np.int64)).to(dev)


def _accumulate(torch, s, ref, near, prox, layers, records=None, with_weight=True, with_counts=True, check_cells=True, **kw):
    """the layers through rsdsfm_superres_accumulate_dev one after another on guarded planes, the cells preset to 0xFFFF and the outputs never
    preset; after every step that is not the last the cells are compared with the definition's, and the last launch must leave them as they
    were.  -> the collected outputs"""
    dev = torch.device("cuda", 0)
    rows, cols = prox.shape
    ch = 1 if ref.ndim == 2 else 3
    L = len(layers)
    d_ref = [_guarded(torch, dev, a) for a in (ref, near, prox)]
    d_l = [[_guarded(torch, dev, a) for a in layer] for layer in layers]
    d_rec = [_record(torch, dev, records[j] if records is not None else None) for j in range(L)]
    d_cells, cells_guard = _cells(torch, dev, rows, cols, ch)
    planes, cnt = _outputs(torch, dev, ref.shape, (rows, cols))
    torch.cuda.synchronize()
    outs = dict(d_image_out=planes[0][0].data_ptr(), d_mask_out=planes[1][0].data_ptr(), d_weight=planes[2][0].data_ptr() if with_weight else None,
                d_counts3=cnt[1:].data_ptr() if with_counts else None)
    rp = [d.data_ptr() for d, _ in d_ref]
    if L == 0:
        s.superres_accumulate_dev(*rp, None, None, None, ch, rows, cols, None, True, True, **outs, **kw)
    want_cells = np.full((rows, cols, ch + 1), 0xFFFF, dtype=np.uint16)
    for j, dl in enumerate(d_l):
        s.superres_accumulate_dev(*rp, *[d.data_ptr() for d, _ in dl], ch, rows, cols, d_cells.data_ptr(), j == 0, j == L - 1,
                                  d_sums8=d_rec[j].data_ptr() if d_rec[j] is not None else None, **outs, **kw)
        if j < L - 1:  # the last launch does not write the cells
            want_cells = spec.step(None if j == 0 else want_cells, ref, near, prox, *layers[j], j == 0, records[j] if records is not None else None,
                                   kw.get("min_overlap", 0) or spec.MIN_OVERLAP_DEFAULT, kw.get("gain_mode", 0), kw.get("strength", 0) or spec.STRENGTH_DEFAULT)
        if check_cells or j >= L - 2:
            s.synchronize()
            assert np.array_equal(_cells_host(d_cells, rows, cols, ch), want_cells), ("cells after step", j, L)
    s.synchronize()
    for (d, _), a in zip(d_ref, (ref, near, prox)):  # the inputs are only read
        assert np.array_equal(d.cpu().numpy(), a)
    for dl, layer in zip(d_l, layers):
        for (d, _), a in zip(dl, layer):
            assert np.array_equal(d.cpu().numpy(), a)
    if L == 0:
        assert (d_cells.cpu().numpy() == 0xFF).all()
    guards = [g for _, g in d_ref] + [cells_guard] + [g for dl in d_l for _, g in dl]
    return _collect(planes, cnt, guards, with_weight, with_counts)


@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_accumulate_equals_the_definition(rsdsfm, arith, channels):
    """every shape of the denoise's ACC_SHAPES, 1, 2 and 14 layers (first and last together, apart, and with mid steps between), no layer;
    proximity planes with empty, full and mixed words and every value 1 .. 16, random bytes where they are 0; records that drive each gain
    clamp, a plain gain, too small an overlap, and no record; the cells after every step; with and without the weight plane and the counters"""
    import torch

    seen = np.zeros(3, dtype=np.int64)
    rec = cases.records(channels)
    keys = ["plain", "low", "high", "small", "zero", None]
    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in cases.ACC_SHAPES:
            ref, near, prox = cases.reference(*shape, channels)
            for L in cases.ACC_LAYERS:
                ls = cases.layers(ref, *shape, channels, L)
                recs = [rec[k] if k else None for k in (keys * 3)[:L]]
                strength = {1: 12, 2: 40, 14: 25}[L]
                got = _accumulate(torch, s, ref, near, prox, ls, recs, strength=strength, check_cells=L <= 2 or shape in ((17, 65), (37, 67)))
                want = spec.accumulate(ref, near, prox, ls, recs, strength=strength)
                _same(got, want, (shape, L))
                seen += np.array(want["counts"])
            _same(_accumulate(torch, s, ref, near, prox, []), spec.accumulate(ref, near, prox, []), (shape, 0))
            ls = cases.layers(ref, *shape, channels, 2, seed=1)
            want = spec.accumulate(ref, near, prox, ls, None, gain_mode=1, min_overlap=7)
            for with_weight, with_counts in ((False, True), (True, False), (False, False)):
                _same(_accumulate(torch, s, ref, near, prox, ls, None, with_weight, with_counts, gain_mode=1, min_overlap=7), want, shape, with_weight, with_counts)
        assert rsdsfm.superres_accumulate_launches() == 1
    assert (seen > 0).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_every_gain_and_the_largest_sums(rsdsfm, channels):
    """one layer per record of the denoise's records with and without gain_mode 1 and with a min_overlap above the record's count; fourteen
    layers of 255 at proximity 16 on a reference of 255: n = 240, s = 61 200 in every cell"""
    import torch

    with rsdsfm.Solver(0) as s:
        ref, near, prox = cases.reference(33, 129, channels, seed=2)
        ls = cases.layers(ref, 33, 129, channels, 1, seed=2)
        for key, r in cases.records(channels).items():
            for kw in (dict(), dict(gain_mode=1), dict(min_overlap=6000)):
                _same(_accumulate(torch, s, ref, near, prox, ls, [r], strength=60, **kw), spec.accumulate(ref, near, prox, ls, [r], strength=60, **kw), (key, kw))
        shape = (17, 65) if channels == 1 else (17, 65, 3)
        sat, full = np.full(shape, 255, dtype=np.uint8), np.full((17, 65), 16, dtype=np.uint8)
        got = _accumulate(torch, s, sat, sat, full, [(sat, sat, full)] * 14, check_cells=False)
        assert (got["image"] == 255).all() and (got["weight"] == 240).all() and got["counts"] == [0, 0, 17 * 65]


@pytest.mark.parametrize("channels", [1, 3])
def test_the_impulse_shows_the_3x3_footprint_across_tile_borders(rsdsfm, channels):
    """reference and layer equal (bilinear planes) but for one pixel, at every corner and edge midpoint of every tile and of the frame: with
    h = 1 and every proximity 16 the weight plane is 16 on the 3 x 3 window about the pixel (inside the frame) and 32 everywhere else"""
    import torch

    with rsdsfm.Solver(0) as s:
        for rows, cols in ((33, 129), (17, 65)):
            ref, near, _ = cases.reference(rows, cols, channels, seed=3)
            full = np.full((rows, cols), 16, dtype=np.uint8)
            positions = cases.impulse_positions(rows, cols)
            assert {(0, 0), (rows - 1, cols - 1), (15, 63), (16, 64), (15, 64), (16, 63), (8, 64), (16, 32)} <= set(positions)
            for y, x in positions:
                layer = ref.copy()
                layer[y, x] = layer[y, x] ^ 0x40  # |d| = 64 in every channel
                got = _accumulate(torch, s, ref, near, full, [(layer, near, full)], strength=1, with_counts=False, check_cells=False)
                want = np.full((rows, cols), 32, dtype=np.uint8)
                want[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 16
                assert np.array_equal(got["weight"], want), (rows, cols, y, x)
                _same(got, spec.accumulate(ref, near, full, [(layer, near, full)], strength=1), (y, x), counts=False)


def test_the_host_convenience_of_the_accumulate(rsdsfm):
    ref, near, prox = cases.reference(37, 67, 3)
    ls = cases.layers(ref, 37, 67, 3, 3)
    recs = [cases.records(3)["plain"], None, cases.records(3)["low"]]
    with rsdsfm.Solver(0) as s:
        img, mask, w, counts = s.superres_accumulate(ref, near, prox, ls, recs, strength=30)
        _same(dict(image=img, mask=mask, weight=w, counts=counts.tolist()), spec.accumulate(ref, near, prox, ls, recs, strength=30))
        img, mask, w, counts = s.superres_accumulate(ref, near, prox, [])
        _same(dict(image=img, mask=mask, weight=w, counts=counts.tolist()), spec.accumulate(ref, near, prox, []))


def test_accumulate_argument_errors(rsdsfm):
    """every refusal returns RSDSFM_ERR_INVALID and enqueues nothing: the outputs and the cells keep their sentinel; after a refused call the
    same call without the fault goes through"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    u8 = lambda value, *shape: torch.full(shape, value, dtype=torch.uint8, device=dev)
    ref, rnear, rprox = u8(9, rows, cols, 3), u8(20, rows, cols, 3), u8(4, rows, cols)
    lay, lnear, lprox = u8(9, rows, cols, 3), u8(40, rows, cols, 3), u8(12, rows, cols)
    out, omask, wplane = u8(GUARD, rows, cols + 4, 3), u8(GUARD, rows, cols + 4), u8(GUARD, rows, cols + 4)
    cells = torch.full((rows, cols + 4, 4), 0x7BCD, dtype=torch.int16, device=dev)
    counts = torch.full((5,), -1, dtype=torch.int64, device=dev)
    rec = torch.zeros(9, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        def acc(R=ref.data_ptr(), RN=rnear.data_ptr(), qR=rprox.data_ptr(), L=lay.data_ptr(), LN=lnear.data_ptr(), qL=lprox.data_ptr(), ch=3, r=rows, c=cols,
                cl=cells.data_ptr(), first=1, last=1, rc=rec.data_ptr(), mo=0, gm=0, h=12, o=out.data_ptr(), k=omask.data_ptr(), wp=wplane.data_ptr(),
                cnt=counts[1:].data_ptr()):
            return s.superres_accumulate_dev(R, RN, qR, L, LN, qL, ch, r, c, cl, first, last, rc, mo, gm, h, o, k, wp, cnt)

        bads = (dict(R=0), dict(RN=0), dict(qR=0), dict(L=0), dict(LN=0), dict(qL=0), dict(L=0, LN=0), dict(L=0, LN=0, qL=0, first=0), dict(L=0, LN=0, qL=0, last=0),
                dict(o=0), dict(k=0), dict(cl=0, first=0), dict(cl=0, last=0), dict(R=ref.data_ptr() + 1), dict(RN=rnear.data_ptr() + 2), dict(qR=rprox.data_ptr() + 2),
                dict(L=lay.data_ptr() + 3), dict(LN=lnear.data_ptr() + 1), dict(qL=lprox.data_ptr() + 1), dict(o=out.data_ptr() + 1), dict(k=omask.data_ptr() + 2),
                dict(wp=wplane.data_ptr() + 3), dict(cl=cells.data_ptr() + 4), dict(cnt=counts.data_ptr() + 4), dict(rc=rec.data_ptr() + 4), dict(o=ref.data_ptr()),
                dict(k=rprox.data_ptr()), dict(wp=lay.data_ptr()), dict(o=lnear.data_ptr()), dict(o=cells.data_ptr()), dict(k=out.data_ptr()), dict(wp=omask.data_ptr()),
                dict(wp=out.data_ptr()), dict(cl=ref.data_ptr()), dict(cl=lprox.data_ptr()), dict(RN=ref.data_ptr()), dict(qR=ref.data_ptr()), dict(L=ref.data_ptr()),
                dict(LN=lay.data_ptr()), dict(qL=rprox.data_ptr()), dict(ch=2), dict(ch=4), dict(r=1), dict(c=16385), dict(r=16385), dict(c=1), dict(first=2), dict(last=-1),
                dict(h=-1), dict(h=256), dict(gm=2), dict(gm=-1), dict(mo=-1))
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
        # own nearest 20 at 4, the layer's nearest 40 at u = (16 * 12 + 8) >> 4 = 12: (4 * 20 + 12 * 40) / 16 = 35
        flat = out.cpu().numpy().reshape(-1)
        assert (flat[:rows * cols * 3] == 35).all() and (flat[rows * cols * 3:] == GUARD).all() and (omask.cpu().numpy().reshape(-1)[:rows * cols] == 1).all()
        assert counts.cpu().numpy().tolist() == [-1, 0, 0, rows * cols, -1] and (wplane.cpu().numpy().reshape(-1)[:rows * cols] == 16).all()
        # not last: the outputs are not read -- NULL and misaligned ones pass, and nothing is written to them
        acc(last=0, o=0, k=0, wp=0, cnt=0)
        acc(last=0, first=0, o=out.data_ptr() + 1, k=3, wp=5, cnt=counts.data_ptr() + 4)
        s.synchronize()
        c16 = cells.cpu().numpy().view(np.uint16).reshape(-1)[:rows * cols * 4].reshape(-1, 4)
        assert (c16 == [4 * 20 + 24 * 40] * 3 + [28]).all() and counts.cpu().numpy().tolist() == [-1, 0, 0, rows * cols, -1]
        assert (cells.cpu().numpy().view(np.uint16).reshape(-1)[rows * cols * 4:] == 0x7BCD).all()


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
def _clip(torch, dev, case):
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(frames=[tt(x) for x in case["frames"]], maps=[tt(z.T) for z in case["depths"]], Rs=[tt(np.asarray(R).reshape(-1, 9)) for R in case["Rs"]],
                ts=[tt(t) for t in case["ts"]])


def _frame_kw(case):
    return dict(scale=case["scale"], strength=case["strength"], gain=case["gain_mode"] == 0, min_overlap=case["min_overlap"], window=case["window"], mode=case["mode"],
                q5_mode=case["q5_mode"], iterations=case["iterations"])


def _frame(torch, s, case, d=None, q=None, with_weight=True, with_counts=True):
    """one rsdsfm_superres_frame_dev of frame q of a case into guarded, never preset outputs"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = d or _clip(torch, dev, case)
    src, M, m = cases.sources_and_poses(case, q)
    planes, cnt = _outputs(torch, dev, _fine_image_shape(case), _fine(case))
    torch.cuda.synchronize()
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    s.superres_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, planes[0][0].data_ptr(), planes[1][0].data_ptr(),
                         planes[2][0].data_ptr() if with_weight else None, cnt[1:].data_ptr() if with_counts else None, **_frame_kw(case))
    s.synchronize()
    for t, a in zip(d["frames"], case["frames"]):
        assert np.array_equal(t.cpu().numpy(), a)
    return _collect(planes, cnt, (), with_weight, with_counts)


def _parts(torch, s, case):
    """the public calls one after another on planes of the test's own: the own frame's render with its validity plane, then per neighbour the
    render, rsdsfm_seam_overlap_sums_dev and rsdsfm_superres_accumulate_dev"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    orows, ocols = _fine(case)
    ch = 1 if case["frames"][0].ndim == 2 else 3
    S = case["scale"]
    d = _clip(torch, dev, case)
    src, M, m = cases.sources_and_poses(case)
    img = lambda: torch.full(_fine_image_shape(case), GUARD, dtype=torch.uint8, device=dev)
    pl = lambda: torch.full((orows, ocols), GUARD, dtype=torch.uint8, device=dev)
    own = dict(bil=img(), near=img(), prox=pl(), valid=pl())
    lay = dict(bil=img(), near=img(), prox=pl())
    d_cells = torch.full((orows, ocols, ch + 1), -1, dtype=torch.int16, device=dev)
    d_rec = torch.full((8,), -1, dtype=torch.int64, device=dev)
    planes, cnt = _outputs(torch, dev, _fine_image_shape(case), (orows, ocols))
    torch.cuda.synchronize()
    kw = dict(window=case["window"], mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    arg = lambda k: (d["frames"][src[k]].data_ptr(), ch, d["maps"][src[k]].data_ptr(), d["Rs"][src[k]].data_ptr(), d["ts"][src[k]].data_ptr(), case["K"], rows, cols, M[k], m[k], S)
    s.superres_render_dev(*arg(0), own["bil"].data_ptr(), own["near"].data_ptr(), own["prox"].data_ptr(), own["valid"].data_ptr(), **kw)
    outs = dict(d_image_out=planes[0][0].data_ptr(), d_mask_out=planes[1][0].data_ptr(), d_weight=planes[2][0].data_ptr(), d_counts3=cnt[1:].data_ptr())
    acc = dict(min_overlap=case["min_overlap"], gain_mode=case["gain_mode"], strength=case["strength"])
    rp = (own["bil"].data_ptr(), own["near"].data_ptr(), own["prox"].data_ptr())
    if len(src) == 1:
        s.superres_accumulate_dev(*rp, None, None, None, ch, orows, ocols, None, True, True, **acc, **outs)
    for k in range(1, len(src)):
        s.superres_render_dev(*arg(k), lay["bil"].data_ptr(), lay["near"].data_ptr(), lay["prox"].data_ptr(), None, **kw)
        s.seam_overlap_sums_dev(own["bil"].data_ptr(), own["valid"].data_ptr(), lay["bil"].data_ptr(), lay["prox"].data_ptr(), ch, orows, ocols, d_rec.data_ptr())
        s.superres_accumulate_dev(*rp, lay["bil"].data_ptr(), lay["near"].data_ptr(), lay["prox"].data_ptr(), ch, orows, ocols, d_cells.data_ptr(), k == 1, k == len(src) - 1,
                                  d_sums8=d_rec.data_ptr(), **acc, **outs)
    s.synchronize()
    return _collect(planes, cnt), {k: v.cpu().numpy() for k, v in own.items()}


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_every_case_equals_the_definition_and_the_public_calls(oracle, rsdsfm, arith):
    """image, mask, weight plane and the three counts of every fixture case -- the aliased shift scene gray and BGR at scale 2 and 3, a fold clip
    plain and through a zoomed window, gained neighbours with the gain on and off, five sources from the clip's middle and one-sided from its
    first frame, one source alone, the 2 x 2 dense case -- against the golden fixture, and against the public calls made one after another; one
    source alone is its bilinear render.  The cases change the scale on one context: the workspace follows"""
    import torch

    g = np.load(GOLDEN)
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in cases.all_cases(oracle.pose_table):
            n = case["name"] + "/"
            want = dict(image=g[n + "image"], mask=g[n + "mask"], weight=g[n + "weight"], counts=g[n + "counts"].tolist())
            _same(_frame(torch, s, case), want, n)
            parts, own = _parts(torch, s, case)
            _same(parts, want, n + " parts")
            assert np.array_equal(own["valid"], (own["prox"] != 0).astype(np.uint8))
            nsrc = len(cases.sources_and_poses(case)[0])
            if nsrc == 1:
                assert np.array_equal(want["image"], own["bil"]) and np.array_equal(want["mask"], own["valid"]) and np.array_equal(want["weight"], own["prox"])
            rows, cols = case["depths"][0].shape
            assert rsdsfm.superres_launches(rows, cols, case["scale"], nsrc) == nsrc * rsdsfm.stabilize_window_launches(rows, cols) + (1 if nsrc == 1 else 2 * (nsrc - 1))
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
    planes, cnt = _outputs(torch, dev, _fine_image_shape(case), _fine(case))
    torch.cuda.synchronize()
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    with rsdsfm.Solver(0) as s:
        def call(images=pick("frames"), maps=pick("maps"), M=M, m=m, o=planes[0][0].data_ptr(), k=planes[1][0].data_ptr(), w=planes[2][0].data_ptr(),
                 cnt_=cnt[1:].data_ptr(), ch=3, r=rows, c=cols, scale=case["scale"], **kw):
            return s.superres_frame_dev(images, ch, maps, pick("Rs"), pick("ts"), case["K"], r, c, M, m, o, k, w, cnt_, scale=scale, **kw)

        bad_M = M.copy()
        bad_M[1, 0, 0] = np.nan
        params = rsdsfm.SuperresParams()
        params.struct_bytes = 40
        reserved = rsdsfm.SuperresParams()
        reserved.reserved[2] = 1
        bads = (dict(images=[0] + pick("frames")[1:]), dict(maps=pick("maps")[:2] + [0]), dict(images=[]),
                dict(images=pick("frames") * 6, maps=pick("maps") * 6, M=np.tile(M, (6, 1, 1)), m=np.tile(m, (6, 1))), dict(M=bad_M), dict(o=0), dict(k=0),
                dict(o=planes[1][0].data_ptr()), dict(w=planes[0][0].data_ptr()), dict(o=planes[0][0].data_ptr() + 1), dict(cnt_=cnt.data_ptr() + 4),
                dict(o=pick("frames")[2]), dict(ch=2), dict(scale=5), dict(scale=-1), dict(r=8193, scale=2), dict(strength=256), dict(strength=-1), dict(min_overlap=-1),
                dict(window=(0, 0, rows + 1, cols)), dict(window=(1, 1, 0, 4)), dict(iterations=17), dict(params=params), dict(params=reserved))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        for (p, gd) in planes:
            assert (p.cpu().numpy() == GUARD).all() and (gd.cpu().numpy() == GUARD).all()
        assert cnt.cpu().numpy().tolist() == [-1] * 5
        call(strength=case["strength"], min_overlap=case["min_overlap"])
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
    outs = [_outputs(torch, dev, _fine_image_shape(case), _fine(case)) for _ in range(ns)]
    torch.cuda.synchronize()
    ptrs = lambda a: [x.data_ptr() for x in a]
    r = s.superres_video_dev(ptrs(d["frames"]), rows, cols, ch, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"], case["c_path"],
                             case["scales"], [p[0][0].data_ptr() for p, _ in outs], [p[1][0].data_ptr() for p, _ in outs],
                             [p[2][0].data_ptr() for p, _ in outs] if with_weights else None, want_counts=want_counts, radius=case["radius"], **_frame_kw(case))
    s.synchronize()
    got = []
    for q, (planes, cnt) in enumerate(outs):
        one = _collect(planes, cnt, (), with_weights, False)
        one["counts"] = r["counts"][q].tolist() if want_counts else None
        got.append(one)
    return got, d


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_clip_call_equals_the_frame_calls(oracle, rsdsfm, arith):
    """three sources (radius 1) and five (radius 2, the first and last frames with one-sided neighbours; the aliased shift scene, whose path is
    the chain itself, and a smooth clip on a path of its own) and one source alone: every frame of the clip call is the frame call's, which is
    the definition's; without the counters and the weight planes the call only enqueues"""
    import torch

    every = {c["name"]: c for c in cases.all_cases(oracle.pose_table)}
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in (every["gained"], every["five-middle"], every["shift-bgr-x2-0"], every["one-source"]):
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
        outs = [_outputs(torch, dev, _fine_image_shape(case), _fine(case)) for _ in range(5)]
        torch.cuda.synchronize()
        ptrs = lambda a: [x.data_ptr() for x in a]
        bad_scales = case["scales"].copy()
        bad_scales[4] = 0.0

        def call(scales=case["scales"], o=None, **kw):
            return s.superres_video_dev(ptrs(d["frames"]), rows, cols, 1, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"],
                                        case["c_path"], scales, o or [p[0][0].data_ptr() for p, _ in outs], [p[1][0].data_ptr() for p, _ in outs], None, **kw)

        for bad in (dict(scales=bad_scales), dict(radius=8), dict(radius=-1), dict(strength=300), dict(scale=5), dict(o=[outs[0][0][0][0].data_ptr()] * 4 + [0]),
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
def test_evaluate_real_sequence_with_superres(rsdsfm, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, superres=scale or (scale, K)) adds exactly superres, superres_masks and superres_counts and the
    files superres_<p>.png and superres.csv, and frame 0 is the frame call's on the clip's own outputs; without the keyword every key and file
    is what it was"""
    import torch

    from test_gpu_stabilize_search import TRIALS, plain_clip

    frames, rows, cols, K, gamma, seeds, _ = plain_clip(rsdsfm)
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
    n = len(frames) - 1
    dev = torch.device("cuda", 0)
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, superres=(2, 1), out_dir=str(tmp_path / "with"), **kw)
        plain = ev(s, frames, out_dir=str(tmp_path / "without"), **kw)
        ps, o = out["path_smoothed"], out["pairs"]
        src, _, M0, m0, _, _ = rsdsfm.retime_poses(out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], 0.0, nsources=n)
        nb, _, Mn, mn = rsdsfm.neighbour_poses(out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], 0, 1)
        order = list(src) + list(nb)
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_f, d_z = [tt(frames[q]) for q in order], [tt(np.asarray(o[q]["depth_map"]).T) for q in order]
        d_R, d_t = [tt(np.asarray(o[q]["R"]).reshape(-1, 9)) for q in order], [tt(o[q]["t"]) for q in order]
        planes, cnt = _outputs(torch, dev, (2 * rows, 2 * cols) + tuple(frames[0].shape[2:]), (2 * rows, 2 * cols))
        torch.cuda.synchronize()
        ptrs = lambda a: [x.data_ptr() for x in a]
        s.superres_frame_dev(ptrs(d_f), 3, ptrs(d_z), ptrs(d_R), ptrs(d_t), K, rows, cols, np.concatenate([M0, Mn]), np.concatenate([m0, mn]), planes[0][0].data_ptr(),
                             planes[1][0].data_ptr(), planes[2][0].data_ptr(), cnt[1:].data_ptr(), scale=2)
        s.synchronize()
        one = _collect(planes, cnt)
    new = {"superres", "superres_masks", "superres_counts"}
    assert set(out) == set(plain) | new
    assert len(out["superres"]) == len(out["superres_masks"]) == n and out["superres_counts"].shape == (n, 3)
    _same(dict(image=out["superres"][0], mask=out["superres_masks"][0], counts=out["superres_counts"][0].tolist()), one, weight=False)
    for p in range(n):
        assert out["superres"][p].shape == (2 * rows, 2 * cols) + tuple(frames[0].shape[2:]) and out["superres_counts"][p].sum() == 4 * rows * cols
    assert sum(int(c[2]) for c in out["superres_counts"]) > 0  # something was merged
    for k in plain:
        if k not in ("pairs", "path_smoothed", "links"):
            assert np.asarray(out[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    with_files, without_files = set(os.listdir(str(tmp_path / "with"))), set(os.listdir(str(tmp_path / "without")))
    assert with_files == without_files | {"superres_%d.png" % p for p in range(n)} | {"superres.csv"}
    lines = open(str(tmp_path / "with" / "superres.csv")).read().split()
    assert lines[0] == "pair,unset,own_only,merged" and len(lines) == 1 + n
    assert lines[1].split(",") == ["0"] + [str(int(x)) for x in out["superres_counts"][0]]
