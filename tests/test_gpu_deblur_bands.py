"""GPU: the sharpness transfer per scanline band (include/rsdsfm_deblur.h, "per scanline band") bit for bit against its definition
(tests/deblur_bands_spec_numpy.py) in both library builds, at the smallest shapes and band heights at which the kernels can go wrong
(tests/deblur_bands_cases.SHAPES): the band records and their sum, the band accumulate's cells after every step and its outputs, one band
against the unbanded call, the mid launch whose taus are 0, an impulse on either side of a band border, the frame call against the definition,
the golden fixture and the public calls made one after another, the clip call against the frame calls with its band taus, the refusals and
their texts, the evaluation's third element.  Every record, cell and output buffer is a guarded_planes.Plane: exactly the alignment the header
admits, guard bytes on either side, outputs never preset -- a record read or write outside NB x 32 B, or a byte outside a plane, shows as a
failed comparison."""
import os

import numpy as np
import pytest

import deblur_bands_cases as bcases
import deblur_bands_spec_numpy as bands
import deblur_cases as cases
import deblur_spec_numpy as spec
from guarded_planes import fresh
from test_gpu_deblur import _clip, _dev, _frame_kw, _Outs, _plane, _same, _sharpness, _words

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_deblur_bands_v1.npz")
TAU0 = [5000, 1000, 1000, 0]   # deblur_cases.sharp_records()["equal"]: tau 0 at every margin
TAU32 = [5000, 1000, 3000, 0]  # "cap": tau 32


def _band_records(s, ref, rmask, layer, lmask, band_rows, record=None, **kw):
    """one rsdsfm_deblur_band_sharpness_dev on guarded planes -> (NB, 4) uint64; the inputs are verified unchanged"""
    ch = 1 if ref.ndim == 2 else 3
    planes = [_plane(a) for a in (ref, rmask, layer, lmask)]
    d_rec = _words(record) if record is not None else None
    d_T = fresh((bands.nbands(rmask.shape[0], band_rows), 4), np.uint64, 8, 16, _dev())
    s.deblur_band_sharpness_dev(planes[0].ptr, planes[1].ptr, planes[2].ptr, planes[3].ptr, ch, *rmask.shape, band_rows, d_T.ptr, d_rec.ptr if d_rec else None, **kw)
    s.synchronize()
    assert all(p.unchanged() for p in planes) and (d_rec is None or d_rec.unchanged())
    return d_T.get()


def _run(s, case, band_rows, band_records=None, with_weight=True, with_counts=True):
    """the case's layers through the sharpness call (where no records are given) and the accumulate call one after another on guarded planes,
    the cells preset to 0xFFFF and the outputs never preset; band_rows None: the unbanded pair of calls
    -> the collected outputs plus records (one array per layer) and cells (after every step that is not the last)"""
    ref, rmask, layers, records, kw = case["ref"], case["rmask"], case["layers"], case["records"], case["kw"]
    rows, cols = rmask.shape
    ch = 1 if ref.ndim == 2 else 3
    L = len(layers)
    nb = bands.nbands(rows, band_rows) if band_rows else 1
    d_ref, d_rm = _plane(ref), _plane(rmask)
    d_l = [(_plane(i), _plane(m)) for i, m in layers]
    d_rec = [_words(records[j]) if records[j] is not None else None for j in range(L)]
    d_T = [_words(band_records[j]) if band_records is not None else fresh((nb, 4) if band_rows else (4,), np.uint64, 8, 16, _dev()) for j in range(L)]
    d_cells = _words(np.full((rows, cols, ch + 1), 0xFFFF, dtype=np.uint16), np.uint16)
    outs = _Outs(ref.shape, (rows, cols))
    okw = outs.kw(with_weight, with_counts)
    gains = dict(min_overlap=kw.get("min_overlap", 0), gain_mode=kw.get("gain_mode", 0))
    if L == 0:
        if band_rows:
            s.deblur_band_accumulate_dev(d_ref.ptr, d_rm.ptr, None, None, ch, rows, cols, band_rows, None, True, True, **kw, **okw)
        else:
            s.deblur_accumulate_dev(d_ref.ptr, d_rm.ptr, None, None, ch, rows, cols, None, True, True, **kw, **okw)
    trail = []
    for j, (d_i, d_m) in enumerate(d_l):
        rec_ptr = d_rec[j].ptr if d_rec[j] else None
        if band_rows:
            if band_records is None:
                s.deblur_band_sharpness_dev(d_ref.ptr, d_rm.ptr, d_i.ptr, d_m.ptr, ch, rows, cols, band_rows, d_T[j].ptr, rec_ptr, **gains)
            s.deblur_band_accumulate_dev(d_ref.ptr, d_rm.ptr, d_i.ptr, d_m.ptr, ch, rows, cols, band_rows, d_cells.ptr, j == 0, j == L - 1, d_T[j].ptr, rec_ptr, **kw, **okw)
        else:
            if band_records is None:
                s.deblur_sharpness_dev(d_ref.ptr, d_rm.ptr, d_i.ptr, d_m.ptr, ch, rows, cols, d_T[j].ptr, rec_ptr, **gains)
            s.deblur_accumulate_dev(d_ref.ptr, d_rm.ptr, d_i.ptr, d_m.ptr, ch, rows, cols, d_cells.ptr, j == 0, j == L - 1, d_T[j].ptr, rec_ptr, **kw, **okw)
        s.synchronize()
        trail.append(d_cells.get())
    assert d_ref.unchanged() and d_rm.unchanged() and all(a.unchanged() and b.unchanged() for a, b in d_l)  # the inputs are only read
    assert all(r is None or r.unchanged() for r in d_rec) and (band_records is None or all(t.unchanged() for t in d_T))
    if L == 0:
        assert d_cells.unchanged()
    return dict(outs.collect(with_weight, with_counts), records=[t.get() for t in d_T], cells=trail)


def _check_against_the_definition(got, want, name, weight=True, counts=True):
    _same(got, want, name, weight, counts)
    L = len(want["cells"])
    assert np.array_equal(np.array(got["records"]).reshape(want["band_records"].shape), want["band_records"]), name
    for j in range(L - 1):  # the last launch does not write the cells
        assert np.array_equal(got["cells"][j], want["cells"][j]), (name, "cells after step", j)
    if L > 1:
        assert np.array_equal(got["cells"][L - 1], want["cells"][L - 2]), (name, "the last launch left the cells as they were")


# ---------------------------------------------------------------------------------------------------
# the band records
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_band_records_equal_the_definition_and_sum_to_the_frame_record(rsdsfm, arith, channels):
    with rsdsfm.Solver(0, arith=arith) as s:
        for i, (rows, cols, H) in enumerate(bcases.SHAPES):
            case = bcases.accumulate_case(rows, cols, H, channels, seed=i)
            for (limg, lmask), rec in zip(case["layers"][:2], case["records"][:2]):
                T = _band_records(s, case["ref"], case["rmask"], limg, lmask, H, rec)
                assert T.tolist() == bands.band_sharpness(case["ref"], case["rmask"], limg, lmask, H, rec).tolist(), case["name"]
                assert T.sum(axis=0).tolist() == _sharpness(s, case["ref"], case["rmask"], limg, lmask, rec).tolist(), case["name"]


@pytest.mark.parametrize("channels", [1, 3])
def test_an_impulse_on_either_side_of_a_band_border_changes_exactly_its_records(rsdsfm, channels):
    """33 x 66 at H = 16, flat images: one bright layer pixel in row 15 (the last of band 0) puts its four pairs into band 0 -- the vertical pair
    across the border belongs to the upper band -- and one in row 16 puts the pair with row 15 into band 0 and its other three into band 1; at
    column 63 and 64, either side of a tile border, and at the frame's last column"""
    rows, cols, H = 33, 66, 16
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    flat, full = np.full(shape, 100, dtype=np.uint8), np.ones((rows, cols), dtype=np.uint8)
    d2 = (100 * channels) ** 2
    with rsdsfm.Solver(0) as s:
        base = _band_records(s, flat, full, flat, full, H)
        npairs = lambda r: r * (cols - 1) + r * cols  # of a band of r rows with a row below it
        assert base.tolist() == [[npairs(16), 0, 0, 0], [npairs(16), 0, 0, 0], [cols - 1, 0, 0, 0]]
        for x in (63, 64, 20, cols - 1):
            sides = 1 if x == cols - 1 else 2
            for y, want in ((15, [(2 + sides) * d2, 0, 0]), (16, [d2, (1 + sides) * d2, 0]), (31, [0, (2 + sides) * d2, 0]), (32, [0, d2, sides * d2])):
                layer = flat.copy()
                layer[y, x] = 200
                T = _band_records(s, flat, full, layer, full, H)
                assert T.tolist() == bands.band_sharpness(flat, full, layer, full, H).tolist(), (y, x)
                assert T[:, 2].tolist() == want and T[:, 0].tolist() == base[:, 0].tolist() and not T[:, 1].any() and not T[:, 3].any(), (y, x)


# ---------------------------------------------------------------------------------------------------
# the band accumulate
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_band_accumulate_equals_the_definition(rsdsfm, arith, channels):
    """three layers (first, mid, last) at every shape and band height against the golden fixture's case, the cells after every step; two layers
    (first, last), one (first and last) and none; without the weight plane, without the counters"""
    g = np.load(GOLDEN)
    with rsdsfm.Solver(0, arith=arith) as s:
        for i, (rows, cols, H) in enumerate(bcases.SHAPES):
            case = bcases.accumulate_case(rows, cols, H, channels, seed=i)
            want = bcases.run_accumulate(case)
            n = case["name"] + "/"
            assert np.array_equal(want["image"], g[n + "image"]) and want["band_taus"] == g[n + "band_taus"].tolist()
            _check_against_the_definition(_run(s, case, H), want, case["name"])
        case = bcases.accumulate_case(50, 70, 16, channels)
        for L, with_weight, with_counts in ((2, False, True), (1, True, False), (0, True, True)):
            part = dict(case, layers=case["layers"][:L], records=case["records"][:L])
            want = bcases.run_accumulate(part)
            _check_against_the_definition(_run(s, part, 16, None, with_weight, with_counts), want, (case["name"], L), with_weight, with_counts)


@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_one_band_is_the_unbanded_accumulate_byte_for_byte(rsdsfm, arith, channels):
    case = bcases.accumulate_case(40, 64, 48, channels, seed=4)
    with rsdsfm.Solver(0, arith=arith) as s:
        banded, plain = _run(s, case, 48), _run(s, case, None)
        _same(banded, plain, case["name"])
        assert np.array_equal(np.array(banded["records"]).reshape(-1, 4), np.array(plain["records"]).reshape(-1, 4))
        assert len(banded["cells"]) == 3 and all(np.array_equal(a, b) for a, b in zip(banded["cells"], plain["cells"]))
        assert any(rsdsfm.deblur_tau(T, case["kw"]["margin"], case["kw"]["min_pairs"]) for T in plain["records"])  # something was transferred


@pytest.mark.parametrize("channels", [1, 3])
def test_a_mid_launch_with_zero_taus_leaves_the_cells_untouched(rsdsfm, channels):
    """50 x 70 at H = 16, the cells those of the own frame: with every band's tau 0 a mid launch changes no cell byte and writes no output; with
    taus [0, 0, 32, 32] the rows both of whose surrounding bands have tau 0 (rows 0 .. 24) keep their cells and the others are the definition's"""
    case = bcases.accumulate_case(50, 70, 16, channels)
    ref, rmask, (limg, lmask), kw = case["ref"], case["rmask"], case["layers"][0], case["kw"]
    rows, cols = rmask.shape
    own = spec.step(None, ref, rmask, None, None, True)
    sk = bcases.spec_kw(kw)
    with rsdsfm.Solver(0) as s:
        for recs in ([TAU0] * 4, [TAU0, TAU0, TAU32, TAU32]):
            planes = [_plane(a) for a in (ref, rmask, limg, lmask)]
            d_T, d_cells = _words(np.array(recs, dtype=np.uint64)), _words(own, np.uint16)
            outs = _Outs(ref.shape, (rows, cols))
            s.deblur_band_accumulate_dev(planes[0].ptr, planes[1].ptr, planes[2].ptr, planes[3].ptr, channels, rows, cols, 16, d_cells.ptr, False, False, d_T.ptr, None, **kw,
                                         **outs.kw())
            s.synchronize()
            assert outs.untouched() and d_T.unchanged() and all(p.unchanged() for p in planes)
            t_rows = bands.row_taus(bands.band_taus(recs, sk["margin"], sk["min_pairs"]), 16, rows)
            want = bands.step(own, ref, rmask, limg, lmask, False, t_rows, None, sk["min_overlap"], sk["gain_mode"], sk["strength"], sk["gate_mode"])
            assert np.array_equal(d_cells.get(), want)
            if recs[2] == TAU0:
                assert d_cells.unchanged()
            else:
                assert (t_rows[:25] == 0).all() and np.array_equal(want[:25], own[:25]) and not np.array_equal(want[25:], own[25:])


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
def _band_frame(torch, s, case, d=None, q=None, with_records=True, band_rows="case"):
    """one rsdsfm_deblur_frame_dev of frame q of a frame case with band_rows into guarded, never preset outputs"""
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    band_rows = case["band_rows"] if band_rows == "case" else band_rows
    nb = bands.nbands(rows, band_rows) if band_rows else 1
    d = d or _clip(torch, case)
    src, M, m = cases.sources_and_poses(case, q)
    outs = _Outs(case["frames"][0].shape, (rows, cols))
    d_T = fresh((max(len(src) - 1, 1), nb, 4), np.uint64, 8, 16, _dev())
    torch.cuda.synchronize()
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    s.deblur_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, *outs.ptrs(), d_T.ptr if with_records else None,
                       band_rows=band_rows, **_frame_kw(case))
    s.synchronize()
    assert with_records or d_T.unchanged()
    return dict(outs.collect(), band_records=d_T.get()[:len(src) - 1])


def _band_parts(torch, s, case):
    """the public calls one after another on planes of the test's own: the own frame's window render onto zeroed planes, then per neighbour the
    render alone onto a zeroed layer, rsdsfm_seam_overlap_sums_dev, rsdsfm_deblur_band_sharpness_dev and rsdsfm_deblur_band_accumulate_dev"""
    dev = _dev()
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    H = case["band_rows"]
    d = _clip(torch, case)
    src, M, m = cases.sources_and_poses(case)
    z = lambda like=None: torch.zeros_like(d["frames"][0]) if like is None else torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
    d_ref, d_rm, d_rs = z(), z(1), z(1)
    d_cells = torch.full((rows, cols, ch + 1), -1, dtype=torch.int16, device=dev)
    d_rec = torch.full((8,), -1, dtype=torch.int64, device=dev)
    d_T = fresh((bands.nbands(rows, H), 4), np.uint64, 8, 16, dev)
    outs = _Outs(case["frames"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    kw = dict(mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    arg = lambda k: (d["frames"][src[k]].data_ptr(), ch, d["maps"][src[k]].data_ptr(), d["Rs"][src[k]].data_ptr(), d["ts"][src[k]].data_ptr(), case["K"], rows, cols, M[k], m[k])
    s.stabilize_window_frame_dev(*arg(0), 1, case["window"], d_ref.data_ptr(), d_rm.data_ptr(), d_rs.data_ptr(), **kw)
    acc = dict(min_overlap=case["min_overlap"], gain_mode=case["gain_mode"], strength=case["strength"], margin=cases.abi_margin(case), min_pairs=case["min_pairs"],
               gate_mode=case["gate_mode"])
    for k in range(1, len(src)):
        d_l, d_lm = z(), z(1)
        torch.cuda.synchronize()
        s.stabilize_window_frame_dev(*arg(k), 2, case["window"], d_l.data_ptr(), d_lm.data_ptr(), **kw)
        s.seam_overlap_sums_dev(d_ref.data_ptr(), d_rs.data_ptr(), d_l.data_ptr(), d_lm.data_ptr(), ch, rows, cols, d_rec.data_ptr())
        s.deblur_band_sharpness_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_l.data_ptr(), d_lm.data_ptr(), ch, rows, cols, H, d_T.ptr, d_rec.data_ptr(), case["min_overlap"],
                                    case["gain_mode"])
        s.deblur_band_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_l.data_ptr(), d_lm.data_ptr(), ch, rows, cols, H, d_cells.data_ptr(), k == 1, k == len(src) - 1,
                                     d_T.ptr, d_rec.data_ptr(), **acc, **outs.kw())
        s.synchronize()  # d_l and d_lm are released at the end of the iteration
    return outs.collect()


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_frame_call_equals_the_definition_and_the_public_calls(rsdsfm, arith):
    """two bands, BGR and gray, and one band: image, mask, weight plane, counts and band records against the golden fixture and against the
    public calls made one after another; without the record array (the workspace's own plane); band_rows 0 is the call without the field"""
    import torch

    g = np.load(GOLDEN)
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in bcases.frame_cases():
            n = case["name"] + "/"
            want = dict(image=g[n + "image"], mask=g[n + "mask"], weight=g[n + "weight"], counts=g[n + "counts"].tolist())
            got = _band_frame(torch, s, case)
            _same(got, want, n)
            assert np.array_equal(got["band_records"], g[n + "band_records"]), n
            taus = [rsdsfm.deblur_band_taus(T, cases.abi_margin(case), case["min_pairs"]).tolist() for T in got["band_records"]]
            assert taus == g[n + "band_taus"].tolist(), n
            _same(_band_parts(torch, s, case), want, n + " parts")
            _same(_band_frame(torch, s, case, with_records=False), want, n + " without the record array")
            rows, cols = case["depths"][0].shape
            assert rsdsfm.deblur_launches(rows, cols, 5) == 5 * rsdsfm.stabilize_window_launches(rows, cols) + 3 * 4
        case = bcases.frame_cases()[0]
        off, absent = _band_frame(torch, s, case, band_rows=0), _band_frame(torch, s, case, band_rows=None)
        want = cases.run_spec(case)
        _same(off, want, "band_rows 0")
        _same(absent, want, "no band_rows")
        assert np.array_equal(off["band_records"][:, 0], want["sharps"]) and np.array_equal(absent["band_records"], off["band_records"])
        assert not np.array_equal(want["image"], g[case["name"] + "/image"])  # and the bands change the frame


# ---------------------------------------------------------------------------------------------------
# the clip call
# ---------------------------------------------------------------------------------------------------
def _band_video(torch, s, case, band_rows, want_counts=True, want_taus=True):
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    ns = len(case["depths"])
    d = _clip(torch, case)
    outs = [_Outs(case["frames"][0].shape, (rows, cols)) for _ in range(ns)]
    torch.cuda.synchronize()
    ptrs = lambda a: [x.data_ptr() for x in a]
    r = s.deblur_video_dev(ptrs(d["frames"]), rows, cols, ch, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"], case["c_path"],
                           case["scales"], [o.image.ptr for o in outs], [o.mask.ptr for o in outs], [o.weight.ptr for o in outs], want_counts=want_counts,
                           want_taus=want_taus, radius=case["radius"], band_rows=band_rows, **_frame_kw(case))
    s.synchronize()
    return r, [o.collect(True, False) for o in outs], d


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_clip_call_equals_the_frame_calls(rsdsfm, arith):
    """five sources at radius 2, two bands: every frame of the clip call is the frame call's, which is the definition's; band_taus and the largest
    band tau in taus are the host functions' on the frame call's records, -1 behind the listed neighbours; with the counts alone; band_rows 0
    gives the unbanded clip with band_taus of one band"""
    import torch

    with rsdsfm.Solver(0, arith=arith) as s:
        for case in bcases.frame_cases()[:2]:
            H = case["band_rows"]
            r, got, d = _band_video(torch, s, case, H)
            assert set(r) == {"counts", "taus", "band_taus"} and r["band_taus"].shape == (5, 6, 2) and r["taus"].shape == (5, 6)
            for q in range(5):
                want = bcases.run_frame(case, q)
                _same(dict(got[q], counts=r["counts"][q].tolist()), want, (case["name"], q))
                one = _band_frame(torch, s, case, d, q)
                _same(one, want, (case["name"], q, "frame"))
                listed = len(want["band_taus"])
                host = [rsdsfm.deblur_band_taus(T, cases.abi_margin(case), case["min_pairs"]).tolist() for T in one["band_records"]]
                assert host == want["band_taus"] and r["band_taus"][q].tolist() == host + [[-1, -1]] * (6 - listed), (case["name"], q)
                assert r["taus"][q].tolist() == [max(t) for t in host] + [-1] * (6 - listed), (case["name"], q)
            assert r["band_taus"][2, :4].max() == 32  # frame 2 is the blurred one
        case = bcases.frame_cases()[1]
        r, got, _ = _band_video(torch, s, case, case["band_rows"], want_taus=False)
        assert set(r) == {"counts"}
        for q in range(5):
            _same(dict(got[q], counts=r["counts"][q].tolist()), bcases.run_frame(case, q), q)
        r0, got0, _ = _band_video(torch, s, case, 0)
        rn, gotn, _ = _band_video(torch, s, case, None)
        assert set(rn) == {"counts", "taus"} and r0["band_taus"].shape == (5, 6, 1)
        assert np.array_equal(r0["taus"], rn["taus"]) and np.array_equal(r0["band_taus"][:, :, 0], rn["taus"]) and np.array_equal(r0["counts"], rn["counts"])
        for q in range(5):
            _same(dict(got0[q], counts=None), dict(gotn[q], counts=None), q, counts=False)
            _same(dict(gotn[q], counts=rn["counts"][q].tolist()), cases.run_spec(case, q), q)


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
BAND_ROWS_TEXT = r"deblur bands: band_rows must be a multiple of 16 in \[16, 16384\]$"
BAND_COUNT_TEXT = r"deblur bands: rows / band_rows gives more than 64 bands \(RSDSFM_DEBLUR_BANDS_MAX\)$"
PARAMS_TEXT = r"rsdsfm_deblur_params: band_rows must be 0 \(off\) or a multiple of 16 in \[16, 16384\]$"


def test_band_call_refusals_have_their_own_texts_and_enqueue_nothing(rsdsfm):
    rows, cols, ch = 33, 66, 3
    case = bcases.accumulate_case(rows, cols, 16, ch, seed=1)
    (limg, lmask), rec = case["layers"][1], case["records"][1]
    planes = [_plane(a) for a in (case["ref"], case["rmask"], limg, lmask)]
    p = [x.ptr for x in planes]
    d_rec = _words(rec)
    d_T = fresh((3, 4), np.uint64, 8, 16, _dev())
    d_cells = _words(np.full((rows, cols, ch + 1), 0xFFFF, dtype=np.uint16), np.uint16)
    outs = _Outs(case["ref"].shape, (rows, cols))
    tall = [_plane(np.zeros((1040, 4) + s, dtype=np.uint8)) for s in ((3,), (), (3,), ())]  # 65 bands at H = 16
    tall_out = _Outs((1040, 4, 3), (1040, 4))
    with rsdsfm.Solver(0) as s:
        sharp = lambda H=16, T=d_T.ptr, sums=d_rec.ptr, pl=p, r=rows, c=cols: s.deblur_band_sharpness_dev(*pl, ch, r, c, H, T, sums)
        acc = lambda H=16, T=d_T.ptr, sums=d_rec.ptr, pl=p, r=rows, c=cols, cells=d_cells.ptr, o=outs: s.deblur_band_accumulate_dev(*pl, ch, r, c, H, cells, True, True, T,
                                                                                                                                     sums, **case["kw"], **o.kw())
        for call in (sharp, acc):
            for H in (8, 24, -16, 16400, 0):
                with pytest.raises(rsdsfm.RsdsfmError, match=BAND_ROWS_TEXT):
                    call(H=H)
            with pytest.raises(rsdsfm.RsdsfmError, match=BAND_COUNT_TEXT):
                call(pl=[x.ptr for x in tall], r=1040, c=4, **(dict(o=tall_out) if call is acc else {}))
        for bad, text in ((dict(T=d_T.ptr + 4), "deblur sharpness: the records must be 8-byte aligned$"), (dict(T=p[0]), "deblur sharpness: the records must be 8-byte aligned$"),
                          (dict(T=d_rec.ptr), "deblur sharpness: the record may not be an input$"), (dict(T=None), "deblur sharpness: null device pointer$"),
                          (dict(sums=d_rec.ptr + 4), "deblur sharpness: the records must be 8-byte aligned$")):
            with pytest.raises(rsdsfm.RsdsfmError, match=text):
                sharp(**bad)
        for bad, text in ((dict(T=d_T.ptr + 4), "deblur accumulate: the cells and the records must be 8-byte aligned$"),
                          (dict(T=outs.counts.ptr), "deblur accumulate: an output may not be an input, a record or the cells$"),
                          (dict(T=d_cells.ptr), "deblur accumulate: the cells may not be an input plane or a record$"),
                          (dict(T=None), "deblur accumulate: a layer needs its band records$")):
            with pytest.raises(rsdsfm.RsdsfmError, match=text):
                acc(**bad)
        s.synchronize()
        assert outs.untouched() and tall_out.untouched() and d_T.unchanged() and d_cells.unchanged()
        # and the faultless calls leave what the definition says
        sharp()
        acc()
        s.synchronize()
        one = dict(case, layers=[(limg, lmask)], records=[rec])
        want = bcases.run_accumulate(one)
        _same(outs.collect(), want)
        assert np.array_equal(d_T.get(), want["band_records"][0]) and d_cells.unchanged()


def test_frame_and_clip_refusals_of_band_rows(rsdsfm):
    import torch

    case = bcases.frame_cases()[0]
    rows, cols = case["depths"][0].shape
    d = _clip(torch, case)
    src, M, m = cases.sources_and_poses(case)
    outs = _Outs(case["frames"][0].shape, (rows, cols))
    clip_outs = [_Outs(case["frames"][0].shape, (rows, cols)) for _ in range(5)]
    d_T = fresh((4, 2, 4), np.uint64, 8, 16, _dev())
    torch.cuda.synchronize()
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    ptrs = lambda a: [x.data_ptr() for x in a]
    with rsdsfm.Solver(0) as s:
        frame = lambda T=d_T.ptr, **kw: s.deblur_frame_dev(pick("frames"), 3, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, *outs.ptrs(), T,
                                                           **dict(_frame_kw(case), **kw))
        video = lambda **kw: s.deblur_video_dev(ptrs(d["frames"]), rows, cols, 3, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"],
                                                case["A_path"], case["c_path"], case["scales"], [o.image.ptr for o in clip_outs], [o.mask.ptr for o in clip_outs], None, **kw)
        for H in (8, 24, -16, 16400):
            for call in (frame, video):
                with pytest.raises(rsdsfm.RsdsfmError, match=PARAMS_TEXT):
                    call(band_rows=H)
        with pytest.raises(rsdsfm.RsdsfmError, match="deblur frame: the sharpness records must be 8-byte aligned and no output$"):
            frame(T=d_T.ptr + 4, band_rows=16)
        with pytest.raises(rsdsfm.RsdsfmError, match="deblur frame: the sharpness records must be 8-byte aligned and no output$"):
            frame(T=outs.counts.ptr, band_rows=16)
        with pytest.raises(rsdsfm.RsdsfmError, match="rsdsfm_deblur_params: radius in"):  # the existing message stays the params' other words'
            frame(band_rows=16, strength=256)
        s.synchronize()
        assert outs.untouched() and d_T.unchanged() and all(o.untouched() for o in clip_outs)
        frame(band_rows=16)
        s.synchronize()
        want = bcases.run_frame(case)
        _same(outs.collect(), want)
        assert np.array_equal(d_T.get(), want["band_records"])


# ---------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------
def test_evaluate_real_sequence_with_band_rows(rsdsfm, tmp_path):
    """a clip of 4 frames of 32 x 64 whose middle frame is blurred in its lower rows: deblur=(2, 24, 16) adds deblur_band_taus and one csv
    column per neighbour and band behind the existing ones, deblur_taus is the largest band tau; without the third element every key, file
    and byte is what it was"""
    from test_gpu_stabilize_search import TRIALS

    rows, cols, gamma = 32, 64, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)
    sc = 4.0 / np.abs(f0).max()
    frames, _, _ = rsdsfm.synth.render_sequence(4, rows, cols, K, v * sc, w * sc, k, gamma, seed=21, blur=[1, bcases.half_widths(rows, 16), 1, 1])
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=[3, 8, 5], stabilize=True, smooth_sigma=1.0)
    n = len(frames) - 1
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, deblur=(2, 24, 16), out_dir=str(tmp_path / "bands"), **kw)
        two = ev(s, frames, deblur=(2, 24), out_dir=str(tmp_path / "two"), **kw)
        off = ev(s, frames, deblur=(2, 24, 0), **kw)
    assert set(out) == set(two) | {"deblur_band_taus"} and set(off) == set(two)
    bt = out["deblur_band_taus"]
    assert bt.shape == (n, 6, 2) and bt.dtype == np.int32 and np.array_equal(bt.max(axis=2), out["deblur_taus"])
    for p in range(n):
        listed = min(p, 2) + min(n - 1 - p, 2)
        assert (bt[p, :listed] >= 0).all() and (bt[p, :listed] <= 32).all() and (bt[p, listed:] == -1).all()
        assert out["deblurred"][p].shape == frames[0].shape and out["deblur_counts"][p].sum() == rows * cols
    for key in two:
        if key not in ("pairs", "path_smoothed", "links"):
            assert np.asarray(off[key]).tobytes() == np.asarray(two[key]).tobytes(), key
            if not key.startswith("deblur"):
                assert np.asarray(out[key]).tobytes() == np.asarray(two[key]).tobytes(), key
    assert set(os.listdir(str(tmp_path / "bands"))) == set(os.listdir(str(tmp_path / "two")))
    head = "pair,unset,own_only,transferred,tau_0,tau_1,tau_2,tau_3,tau_4,tau_5"
    lines, plain = open(str(tmp_path / "bands" / "deblur.csv")).read().split(), open(str(tmp_path / "two" / "deblur.csv")).read().split()
    assert plain[0] == head and len(plain) == 1 + n
    assert lines[0] == head + "," + ",".join("tau_%d_band_%d" % (j, b) for j in range(6) for b in range(2)) and len(lines) == 1 + n
    assert [int(x) for x in lines[1].split(",")[10:]] == bt[0].reshape(-1).tolist()
