"""GPU: the sharpness transfer (include/rsdsfm_deblur.h) bit for bit against its definition (tests/deblur_spec_numpy.py) in both library builds
-- the sharpness record and the accumulate alone at the shapes where the 16 x 64 tile can go wrong, the cells after every step, every branch of
tau through records, an impulse's pairs and its 3 x 3 footprint across tile borders, the tau = 0 mid launch, the frame call on every case of
tests/deblur_cases.py against the golden fixture the CPU suite holds to the definition and against the public calls made one after another, the
clip call against the frame calls with its counts and taus, argument errors, the evaluation's keyword.  Every plane is a guarded_planes.Plane:
exactly the alignment the header admits (4 bytes for planes, 8 for records, cells and counters), guard bytes on either side, outputs never
preset, inputs verified unchanged."""
import os

import numpy as np
import pytest

import deblur_cases as cases
import deblur_spec_numpy as spec
from guarded_planes import GUARD, Plane, fresh

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_deblur_v1.npz")


def _dev():
    import torch

    return torch.device("cuda", 0)


def _plane(a):
    """an input plane, 4-byte aligned and no more"""
    return Plane(np.ascontiguousarray(a), 4, 8, _dev())


def _words(a, dtype=np.uint64):
    """a record, 8-byte aligned and no more"""
    return Plane(np.ascontiguousarray(a, dtype=dtype), 8, 16, _dev())


class _Outs:
    """image, mask and weight plane and the three counters, never preset"""

    def __init__(self, image_shape, plane_shape):
        self.image, self.mask, self.weight = (fresh(s, np.uint8, 4, 8, _dev()) for s in (image_shape, plane_shape, plane_shape))
        self.counts = fresh((3,), np.int64, 8, 16, _dev())

    def ptrs(self, with_weight=True, with_counts=True):
        return self.image.ptr, self.mask.ptr, self.weight.ptr if with_weight else None, self.counts.ptr if with_counts else None

    def kw(self, with_weight=True, with_counts=True):
        return dict(zip(("d_image_out", "d_mask_out", "d_weight", "d_counts3"), self.ptrs(with_weight, with_counts)))

    def untouched(self):
        return all(p.unchanged() for p in (self.image, self.mask, self.weight, self.counts))

    def collect(self, with_weight=True, with_counts=True):
        assert with_weight or self.weight.unchanged()
        assert with_counts or self.counts.unchanged()
        return dict(image=self.image.get(), mask=self.mask.get(), weight=self.weight.get(), counts=self.counts.get().tolist())


def _same(got, want, name="", weight=True, counts=True):
    for k in ("image", "mask") + (("weight",) if weight else ()):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert not counts or list(got["counts"]) == list(want["counts"]), (name, got["counts"], want["counts"])


def _spec_kw(kw):
    """the ABI's words of a call as the definition's values"""
    return dict(min_overlap=kw.get("min_overlap", 0) or spec.MIN_OVERLAP_DEFAULT, gain_mode=kw.get("gain_mode", 0), strength=kw.get("strength", 0) or spec.STRENGTH_DEFAULT,
                margin=spec.margin_value(kw.get("margin", 0)), min_pairs=kw.get("min_pairs", 0) or spec.MIN_PAIRS_DEFAULT, gate_mode=kw.get("gate_mode", 0))


def _sharpness(s, ref, rmask, layer, lmask, record=None, **kw):
    """one rsdsfm_deblur_sharpness_dev on guarded planes -> (4,) uint64; the inputs are verified unchanged"""
    ch = 1 if ref.ndim == 2 else 3
    planes = [_plane(a) for a in (ref, rmask, layer, lmask)]
    d_rec = _words(record) if record is not None else None
    d_T = fresh((4,), np.uint64, 8, 16, _dev())
    s.deblur_sharpness_dev(planes[0].ptr, planes[1].ptr, planes[2].ptr, planes[3].ptr, ch, *rmask.shape, d_T.ptr, d_rec.ptr if d_rec else None, **kw)
    s.synchronize()
    assert all(p.unchanged() for p in planes) and (d_rec is None or d_rec.unchanged())
    return d_T.get()


def _deblur(s, ref, rmask, layers, records=None, sharps=None, with_weight=True, with_counts=True, check_cells=True, **kw):
    """the layers through rsdsfm_deblur_sharpness_dev (where no record is given) and rsdsfm_deblur_accumulate_dev one after another on guarded
    planes, the cells preset to 0xFFFF and the outputs never preset; the sharpness records, and after every step that is not the last the
    cells, are compared with the definition's, and the last launch must leave the cells as they were.  -> the collected outputs"""
    rows, cols = rmask.shape
    ch = 1 if ref.ndim == 2 else 3
    L = len(layers)
    sk = _spec_kw(kw)
    d_ref, d_rm = _plane(ref), _plane(rmask)
    d_l = [(_plane(i), _plane(m)) for i, m in layers]
    d_rec = [_words(records[j]) if records is not None and records[j] is not None else None for j in range(L)]
    d_T = [_words(sharps[j]) if sharps is not None else fresh((4,), np.uint64, 8, 16, _dev()) for j in range(L)]
    d_cells = _words(np.full((rows, cols, ch + 1), 0xFFFF, dtype=np.uint16), np.uint16)
    outs = _Outs(ref.shape, (rows, cols))
    acc = {k: v for k, v in kw.items()}
    if L == 0:
        s.deblur_accumulate_dev(d_ref.ptr, d_rm.ptr, None, None, ch, rows, cols, None, True, True, **acc, **outs.kw(with_weight, with_counts))
    want_cells = np.full((rows, cols, ch + 1), 0xFFFF, dtype=np.uint16)
    taus = []
    for j, (d_i, d_m) in enumerate(d_l):
        rec_ptr = d_rec[j].ptr if d_rec[j] else None
        rec = records[j] if records is not None else None
        if sharps is None:
            s.deblur_sharpness_dev(d_ref.ptr, d_rm.ptr, d_i.ptr, d_m.ptr, ch, rows, cols, d_T[j].ptr, rec_ptr, min_overlap=kw.get("min_overlap", 0), gain_mode=kw.get("gain_mode", 0))
        s.deblur_accumulate_dev(d_ref.ptr, d_rm.ptr, d_i.ptr, d_m.ptr, ch, rows, cols, d_cells.ptr, j == 0, j == L - 1, d_T[j].ptr, rec_ptr, **acc,
                                **outs.kw(with_weight, with_counts))
        s.synchronize()
        T = d_T[j].get()
        if sharps is None:
            assert T.tolist() == spec.sharpness(ref, rmask, layers[j][0], layers[j][1], rec, sk["min_overlap"], sk["gain_mode"]).tolist(), ("sharpness of layer", j)
        taus.append(spec.tau(T, sk["margin"], sk["min_pairs"]))
        if j < L - 1:  # the last launch does not write the cells
            want_cells = spec.step(None if j == 0 else want_cells, ref, rmask, layers[j][0], layers[j][1], j == 0, taus[j], rec, sk["min_overlap"], sk["gain_mode"],
                                   sk["strength"], sk["gate_mode"])
        if check_cells or j >= L - 2:
            assert np.array_equal(d_cells.get(), want_cells), ("cells after step", j, L)
    s.synchronize()
    assert d_ref.unchanged() and d_rm.unchanged() and all(a.unchanged() and b.unchanged() for a, b in d_l)  # the inputs are only read
    assert all(r is None or r.unchanged() for r in d_rec) and (sharps is None or all(t.unchanged() for t in d_T))
    if L == 0:
        assert d_cells.unchanged()
    return dict(outs.collect(with_weight, with_counts), taus=taus)


# ---------------------------------------------------------------------------------------------------
# the sharpness record
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_sharpness_equals_the_definition(rsdsfm, arith, channels):
    """every shape -- one word, odd sizes, one under, exactly one and one over the tile in both directions, rows that start on every byte of a
    dword, 25 workgroups --; masks with empty, full and mixed words and values other than 0 / 1, random bytes under unset mask bytes; a sharp and
    a blurred reference; records that drive each gain clamp, a plain gain, too small an overlap, gain_mode 1 and no record; full masks (the
    largest pair count of the shape)"""
    rec = cases.records(channels)
    with rsdsfm.Solver(0, arith=arith) as s:
        for n, shape in enumerate(cases.ACC_SHAPES):
            blurred, rmask, sharp = cases.blurred_reference(*shape, channels)
            ls = cases.layers(sharp, *shape, channels, 3, seed=n)
            for j, (ref, key, kw) in enumerate(((blurred, None, dict()), (sharp, "plain", dict()), (blurred, "high", dict(min_overlap=7)), (blurred, "low", dict(gain_mode=1)),
                                                (sharp, "small", dict()), (blurred, "low", dict()))):
                r = rec[key] if key else None
                got = _sharpness(s, ref, rmask, *ls[j % 3], r, **kw)
                want = spec.sharpness(ref, rmask, *ls[j % 3], r, kw.get("min_overlap", 0) or spec.MIN_OVERLAP_DEFAULT, kw.get("gain_mode", 0))
                assert got.tolist() == want.tolist(), (shape, j)
            full = np.full(shape, 255, dtype=np.uint8)
            got = _sharpness(s, blurred, full, sharp, full)
            assert got.tolist() == spec.sharpness(blurred, full, sharp, full).tolist() and got[0] == 2 * shape[0] * shape[1] - shape[0] - shape[1] and got[2] > got[1]
        # the largest sums a tile can give: a checkerboard of 0 and 255 in every channel, 765^2 (BGR) per pair
        yy, xx = np.mgrid[0:33, 0:129]
        board = (255 * ((yy + xx) & 1)).astype(np.uint8)
        board = board if channels == 1 else np.stack([board] * 3, axis=-1)
        full = np.ones((33, 129), dtype=np.uint8)
        pairs = 2 * 33 * 129 - 33 - 129
        assert _sharpness(s, board, full, board, full).tolist() == [pairs, pairs * (255 * channels) ** 2, pairs * (255 * channels) ** 2, 0]


@pytest.mark.parametrize("channels", [1, 3])
def test_an_impulse_changes_exactly_its_pairs_across_tile_borders(rsdsfm, channels):
    """reference and layer flat but for one layer pixel 64 brighter in every channel, at every corner and edge midpoint of every tile and of the
    frame: A_R = 0 and A_L = (64 CH)^2 times the pixel's neighbours inside the frame (4, 3 at an edge, 2 at a corner) -- the pair to the right and
    the pair below reach into the next tile, the pairs from the left and from above come out of the previous one; with the pixel's mask byte unset
    those pairs leave the count instead"""
    with rsdsfm.Solver(0) as s:
        for rows, cols in ((33, 129), (17, 65)):
            shape = (rows, cols) if channels == 1 else (rows, cols, 3)
            ref = np.full(shape, 9, dtype=np.uint8)
            full = np.ones((rows, cols), dtype=np.uint8)
            pairs = 2 * rows * cols - rows - cols
            positions = cases.impulse_positions(rows, cols)
            assert {(0, 0), (rows - 1, cols - 1), (15, 63), (16, 64), (15, 64), (16, 63), (8, 64), (16, 32)} <= set(positions)
            for y, x in positions:
                layer = ref.copy()
                layer[y, x] = 73
                nb = (y > 0) + (x > 0) + (y < rows - 1) + (x < cols - 1)
                assert _sharpness(s, ref, full, layer, full).tolist() == [pairs, 0, nb * (64 * channels) ** 2, 0], (rows, cols, y, x)
                hole = full.copy()
                hole[y, x] = 0
                assert _sharpness(s, ref, full, layer, hole).tolist() == [pairs - nb, 0, 0, 0], (rows, cols, y, x)


# ---------------------------------------------------------------------------------------------------
# the accumulate
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_accumulate_equals_the_definition(rsdsfm, arith, channels):
    """every shape, 1, 2 and 7 layers (first and last together, apart, and with mid steps between) and no layer; the taus driven through
    sharpness records (0 by the margin and by min_pairs, 4 .. 31, the cap) and, on a blurred reference, by the sharpness call itself; overlap
    records that drive each gain clamp; the cells after every step; both gate modes; with and without the weight plane and the counters"""
    seen, taus = np.zeros(3, dtype=np.int64), set()
    rec = cases.records(channels)
    keys = ["plain", "low", "high", "small", "zero", None]
    tkeys = ["twice", "margin", "thirty", "above_margin", "cap", "few_pairs", "half", "below_cap", "flat_own_1", "big"]
    trec = cases.sharp_records()
    with rsdsfm.Solver(0, arith=arith) as s:
        for n, shape in enumerate(cases.ACC_SHAPES):
            blurred, rmask, sharp = cases.blurred_reference(*shape, channels)
            for L in cases.ACC_LAYERS:
                ls = cases.layers(sharp, *shape, channels, L)
                recs = [rec[k] if k else None for k in (keys * 2)[:L]]
                sharps = [trec[k][0] for k in (tkeys[n % 3:] + tkeys)[:L]]
                kw = {1: dict(strength=24), 2: dict(strength=60, gate_mode=1), 7: dict(strength=255)}[L]
                got = _deblur(s, blurred, rmask, ls, recs, sharps, check_cells=L <= 2 or shape in ((17, 65), (37, 67)), **kw)
                want = spec.deblur(blurred, rmask, ls, recs, sharps, **_spec_kw(kw))
                _same(got, want, (shape, L))
                assert got["taus"] == want["taus"]
                seen += np.array(want["counts"])
                taus |= set(want["taus"])
            _same(_deblur(s, blurred, rmask, []), spec.deblur(blurred, rmask, []), (shape, 0))
            # the records from the sharpness call; min_pairs low enough for the smallest shapes
            ls = cases.layers(sharp, *shape, channels, 2, seed=1)
            kw = dict(gain_mode=1, min_overlap=7, min_pairs=1, margin=-1, strength=40)
            want = spec.deblur(blurred, rmask, ls, None, None, **_spec_kw(kw))
            for with_weight, with_counts in ((True, True), (False, True), (True, False), (False, False)):
                got = _deblur(s, blurred, rmask, ls, None, None, with_weight, with_counts, **kw)
                _same(got, want, shape, with_weight, with_counts)
                assert got["taus"] == want["taus"]
            taus |= set(want["taus"])
    assert (seen > 0).all() and {0, 4, 8, 16, 30, 31, 32} <= taus


@pytest.mark.parametrize("channels", [1, 3])
def test_every_record_case_and_the_largest_sums(rsdsfm, channels):
    """one layer per sharpness record of deblur_cases.sharp_records at the defaults, without a margin, at the largest margin and with other
    min_pairs; seven layers of 255 at the cap on a reference of 255: n = 240, s = 61 200 in every cell"""
    with rsdsfm.Solver(0) as s:
        blurred, rmask, sharp = cases.blurred_reference(33, 129, channels, seed=2)
        ls = cases.layers(sharp, 33, 129, channels, 1, seed=2)
        for key, (T, t) in cases.sharp_records().items():
            for kw in (dict(), dict(margin=-1), dict(margin=64), dict(min_pairs=1), dict(min_pairs=5001), dict(margin=1, strength=90, gate_mode=1)):
                got = _deblur(s, blurred, rmask, ls, None, [T], **kw)
                want = spec.deblur(blurred, rmask, ls, None, [T], **_spec_kw(kw))
                _same(got, want, (key, kw))
                assert got["taus"] == want["taus"] and (kw or want["taus"] == [t])
        shape = (17, 65) if channels == 1 else (17, 65, 3)
        sat, full = np.full(shape, 255, dtype=np.uint8), np.full((17, 65), 200, dtype=np.uint8)
        got = _deblur(s, sat, full, [(sat, full)] * 7, None, [cases.sharp_records()["cap"][0]] * 7, check_cells=False)
        assert (got["image"] == 255).all() and (got["weight"] == 240).all() and got["counts"] == [0, 0, 17 * 65]


@pytest.mark.parametrize("channels", [1, 3])
def test_the_impulse_shows_the_3x3_footprint_across_tile_borders(rsdsfm, channels):
    """reference and layer equal but for one pixel, at every corner and edge midpoint of every tile and of the frame: with h = 1 and tau = 16 the
    weight plane is 16 on the 3 x 3 window about the pixel (inside the frame) and 32 everywhere else -- the definition's, across the tile's borders"""
    T = cases.sharp_records()["twice"][0]
    with rsdsfm.Solver(0) as s:
        for rows, cols in ((33, 129), (17, 65)):
            ref, _ = cases.reference(rows, cols, channels, seed=3)
            full = np.ones((rows, cols), dtype=np.uint8)
            for y, x in cases.impulse_positions(rows, cols):
                layer = ref.copy()
                layer[y, x] = layer[y, x] ^ 0x40  # |d| = 64 in every channel, all of one sign
                got = _deblur(s, ref, full, [(layer, full)], None, [T], strength=1, with_counts=False, check_cells=False)
                want = np.full((rows, cols), 32, dtype=np.uint8)
                want[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 16
                assert np.array_equal(got["weight"], want), (rows, cols, y, x)
                _same(got, spec.deblur(ref, full, [(layer, full)], None, [T], strength=1), (y, x), counts=False)


def test_a_mid_launch_with_tau_zero_leaves_the_cells_untouched(rsdsfm):
    """neither first nor last and a record whose tau is 0 (by the margin, by min_pairs, a duller layer): no cell is written; the same launch with
    tau > 0 writes them.  The cells hold a pattern no step could leave"""
    rows, cols = 37, 67
    blurred, rmask, sharp = cases.blurred_reference(rows, cols, 3)
    (layer, lmask), = cases.layers(sharp, rows, cols, 3, 1)
    planes = [_plane(a) for a in (blurred, rmask, layer, lmask)]
    pattern = (17 * (np.arange(rows * cols * 4) % 201)).astype(np.uint16).reshape(rows, cols, 4)
    pattern[..., 3] = 17  # n = 17 with sums up to 17 * 200: inside the cells' bounds, and nothing a first step leaves
    with rsdsfm.Solver(0) as s:
        for key in ("margin", "equal", "duller", "few_pairs", "flat_both", "big_margin"):
            d_cells, d_T = _words(pattern, np.uint16), _words(cases.sharp_records()[key][0])
            s.deblur_accumulate_dev(planes[0].ptr, planes[1].ptr, planes[2].ptr, planes[3].ptr, 3, rows, cols, d_cells.ptr, False, False, d_T.ptr)
            s.synchronize()
            assert d_cells.unchanged() and d_T.unchanged(), key
        d_cells, d_T = _words(pattern, np.uint16), _words(cases.sharp_records()["twice"][0])
        s.deblur_accumulate_dev(planes[0].ptr, planes[1].ptr, planes[2].ptr, planes[3].ptr, 3, rows, cols, d_cells.ptr, False, False, d_T.ptr)
        s.synchronize()
        want = spec.step(pattern, blurred, rmask, layer, lmask, False, 16)
        assert np.array_equal(d_cells.get(), want) and not np.array_equal(want, pattern)
    assert all(p.unchanged() for p in planes)


def test_the_host_conveniences(rsdsfm):
    blurred, rmask, sharp = cases.blurred_reference(37, 67, 3)
    ls = cases.layers(sharp, 37, 67, 3, 3)
    recs = [cases.records(3)["plain"], None, cases.records(3)["low"]]
    with rsdsfm.Solver(0) as s:
        want = spec.deblur(blurred, rmask, ls, recs, strength=30, min_pairs=100)
        img, mask, w, counts, sharps = s.deblur_accumulate(blurred, rmask, ls, recs, strength=30, min_pairs=100)
        _same(dict(image=img, mask=mask, weight=w, counts=counts.tolist()), want)
        assert np.array_equal(sharps, want["sharps"]) and max(want["taus"]) > 0
        assert s.deblur_sharpness(blurred, rmask, *ls[0], recs[0]).tolist() == want["sharps"][0].tolist()
        given = [cases.sharp_records()[k][0] for k in ("half", "cap", "equal")]
        img, mask, w, counts, sharps = s.deblur_accumulate(blurred, rmask, ls, recs, given, gate_mode=1)
        _same(dict(image=img, mask=mask, weight=w, counts=counts.tolist()), spec.deblur(blurred, rmask, ls, recs, given, gate_mode=1))
        img, mask, w, counts, _ = s.deblur_accumulate(blurred, rmask, [])
        _same(dict(image=img, mask=mask, weight=w, counts=counts.tolist()), spec.deblur(blurred, rmask, []))


def test_accumulate_and_sharpness_argument_errors(rsdsfm):
    """every refusal returns RSDSFM_ERR_INVALID and enqueues nothing: the outputs, the cells and the record keep their guard bytes; after a
    refused call the same call without the fault goes through"""
    rows, cols = 16, 64
    ref, lay = _plane(np.full((rows, cols, 3), 9, dtype=np.uint8)), _plane(np.full((rows, cols, 3), 9, dtype=np.uint8))
    rmask, lmask = _plane(np.ones((rows, cols), dtype=np.uint8)), _plane(np.ones((rows, cols), dtype=np.uint8))
    outs = _Outs((rows, cols, 3), (rows, cols))
    cells = fresh((rows, cols, 4), np.uint16, 8, 16, _dev())
    rec, T, Tout = _words(np.zeros(8)), _words(cases.sharp_records()["cap"][0]), fresh((4,), np.uint64, 8, 16, _dev())
    with rsdsfm.Solver(0) as s:
        def acc(R=ref.ptr, mR=rmask.ptr, L=lay.ptr, mL=lmask.ptr, ch=3, r=rows, c=cols, cl=cells.ptr, first=1, last=1, sh=T.ptr, rc=rec.ptr, mo=0, gm=0, h=24, mg=0, mp=0,
                gt=0, o=outs.image.ptr, k=outs.mask.ptr, wp=outs.weight.ptr, cnt=outs.counts.ptr):
            return s.deblur_accumulate_dev(R, mR, L, mL, ch, r, c, cl, first, last, sh, rc, mo, gm, h, mg, mp, gt, o, k, wp, cnt)

        bads = (dict(R=0), dict(mR=0), dict(L=0), dict(mL=0), dict(L=0, mL=0, first=0), dict(L=0, mL=0, last=0), dict(o=0), dict(k=0), dict(cl=0, first=0), dict(cl=0, last=0),
                dict(sh=0), dict(sh=T.ptr + 4), dict(sh=outs.counts.ptr), dict(R=ref.ptr + 1), dict(mR=rmask.ptr + 2), dict(L=lay.ptr + 3), dict(mL=lmask.ptr + 1),
                dict(o=outs.image.ptr + 1), dict(k=outs.mask.ptr + 2), dict(wp=outs.weight.ptr + 3), dict(cl=cells.ptr + 4), dict(cnt=outs.counts.ptr + 4), dict(rc=rec.ptr + 4),
                dict(o=ref.ptr), dict(k=rmask.ptr), dict(wp=lay.ptr), dict(o=lmask.ptr), dict(o=cells.ptr), dict(k=outs.image.ptr), dict(wp=outs.mask.ptr),
                dict(wp=outs.image.ptr), dict(cl=rec.ptr), dict(mR=ref.ptr), dict(L=ref.ptr), dict(mL=lay.ptr), dict(cnt=T.ptr), dict(cl=T.ptr), dict(ch=2),
                dict(ch=4), dict(r=1), dict(c=16385), dict(r=16385), dict(c=1), dict(first=2), dict(last=-1), dict(h=-1), dict(h=256), dict(gm=2), dict(gm=-1), dict(mo=-1),
                dict(mg=-2), dict(mg=65), dict(mp=-1), dict(gt=2), dict(gt=-1))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                acc(**bad)

        def sharp(R=ref.ptr, mR=rmask.ptr, L=lay.ptr, mL=lmask.ptr, ch=3, r=rows, c=cols, out=Tout.ptr, rc=rec.ptr, mo=0, gm=0):
            return s.deblur_sharpness_dev(R, mR, L, mL, ch, r, c, out, rc, mo, gm)

        sbads = (dict(R=0), dict(mR=0), dict(L=0), dict(mL=0), dict(out=0), dict(out=Tout.ptr + 4), dict(rc=rec.ptr + 4), dict(R=ref.ptr + 1), dict(mL=lmask.ptr + 2),
                 dict(out=rec.ptr), dict(L=ref.ptr), dict(mL=rmask.ptr), dict(ch=2), dict(r=1), dict(c=16385), dict(mo=-1), dict(gm=2))
        for bad in sbads:
            with pytest.raises(rsdsfm.RsdsfmError):
                sharp(**bad)
        s.synchronize()
        assert outs.untouched() and cells.unchanged() and Tout.unchanged() and T.unchanged() and rec.unchanged()  # nothing was enqueued
        for bad in bads[:3]:
            with pytest.raises(rsdsfm.RsdsfmError):
                acc(**bad)
            acc()  # the same call without the fault goes through
        acc(cl=0, wp=None, cnt=None)  # first and last: the cells may be NULL
        s.synchronize()
        assert (outs.image.get() == 9).all() and (outs.mask.get() == 1).all() and (outs.weight.get() == 48).all() and outs.counts.get().tolist() == [0, 0, rows * cols]
        assert cells.unchanged()
        # not last: the outputs are not read -- NULL and misaligned ones pass, and nothing is written to them
        acc(last=0, o=0, k=0, wp=0, cnt=0)
        acc(last=0, first=0, o=outs.image.ptr + 1, k=3, wp=5, cnt=outs.counts.ptr + 4)
        s.synchronize()
        assert (cells.get() == [80 * 9, 80 * 9, 80 * 9, 80]).all() and outs.counts.get().tolist() == [0, 0, rows * cols]
        sharp()
        s.synchronize()
        assert Tout.get().tolist() == [2 * rows * cols - rows - cols, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
def _clip(torch, case):
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return dict(frames=[tt(x) for x in case["frames"]], maps=[tt(z.T) for z in case["depths"]], Rs=[tt(np.asarray(R).reshape(-1, 9)) for R in case["Rs"]],
                ts=[tt(t) for t in case["ts"]])


def _frame_kw(case):
    return dict(strength=case["strength"], margin=cases.abi_margin(case), gate=case["gate_mode"] == 0, gain=case["gain_mode"] == 0, min_overlap=case["min_overlap"],
                min_pairs=case["min_pairs"], window=case["window"], occlusion=case["occlusion"], occlusion_tol_q16=case["tol_q16"], mode=case["mode"], q5_mode=case["q5_mode"],
                iterations=case["iterations"])


def _frame(torch, s, case, d=None, q=None, with_weight=True, with_counts=True, with_records=True):
    """one rsdsfm_deblur_frame_dev of frame q of a case (the context's knob set to the case's) into guarded, never preset outputs"""
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = d or _clip(torch, case)
    src, M, m = cases.sources_and_poses(case, q)
    outs = _Outs(case["frames"][0].shape, (rows, cols))
    d_T = fresh((max(len(src) - 1, 1), 4), np.uint64, 8, 16, _dev())
    torch.cuda.synchronize()
    s.set_occlusion_search(case["search"])
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    s.deblur_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, *outs.ptrs(with_weight, with_counts),
                       d_T.ptr if with_records else None, **_frame_kw(case))
    s.synchronize()
    s.set_occlusion_search(0)
    for t, a in zip(d["frames"], case["frames"]):
        assert np.array_equal(t.cpu().numpy(), a)
    assert with_records and len(src) > 1 or d_T.unchanged()
    return dict(outs.collect(with_weight, with_counts), sharps=d_T.get()[:len(src) - 1])


def _parts(torch, s, case):
    """the public calls one after another on planes of the test's own: the own frame's window render (id 1, with a source plane) onto zeroed
    planes, then per neighbour the render alone onto a zeroed layer, rsdsfm_seam_overlap_sums_dev, rsdsfm_deblur_sharpness_dev and
    rsdsfm_deblur_accumulate_dev"""
    dev = _dev()
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = _clip(torch, case)
    src, M, m = cases.sources_and_poses(case)
    z = lambda like=None: torch.zeros_like(d["frames"][0]) if like is None else torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
    d_ref, d_rm, d_rs = z(), z(1), z(1)
    d_cells = torch.full((rows, cols, ch + 1), -1, dtype=torch.int16, device=dev)
    d_rec, d_T = torch.full((8,), -1, dtype=torch.int64, device=dev), torch.full((4,), -1, dtype=torch.int64, device=dev)
    outs = _Outs(case["frames"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    kw = dict(mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    arg = lambda k: (d["frames"][src[k]].data_ptr(), ch, d["maps"][src[k]].data_ptr(), d["Rs"][src[k]].data_ptr(), d["ts"][src[k]].data_ptr(), case["K"], rows, cols, M[k], m[k])
    s.stabilize_window_frame_dev(*arg(0), 1, case["window"], d_ref.data_ptr(), d_rm.data_ptr(), d_rs.data_ptr(), **kw)
    acc = dict(min_overlap=case["min_overlap"], gain_mode=case["gain_mode"], strength=case["strength"], margin=cases.abi_margin(case), min_pairs=case["min_pairs"],
               gate_mode=case["gate_mode"])
    if len(src) == 1:
        s.deblur_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), None, None, ch, rows, cols, None, True, True, **acc, **outs.kw())
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
        s.deblur_sharpness_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_l.data_ptr(), d_lm.data_ptr(), ch, rows, cols, d_T.data_ptr(), d_rec.data_ptr(), case["min_overlap"],
                               case["gain_mode"])
        s.deblur_accumulate_dev(d_ref.data_ptr(), d_rm.data_ptr(), d_l.data_ptr(), d_lm.data_ptr(), ch, rows, cols, d_cells.data_ptr(), k == 1, k == len(src) - 1,
                                d_T.data_ptr(), d_rec.data_ptr(), **acc, **outs.kw())
        s.synchronize()  # d_l and d_lm are released at the end of the iteration
    s.synchronize()
    return outs.collect(), dict(image=d_ref.cpu().numpy(), mask=d_rm.cpu().numpy())


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_every_case_equals_the_definition_and_the_public_calls(oracle, rsdsfm, arith):
    """image, mask, weight plane, the three counts and the sharpness records of every fixture case -- the blurred own frame, BGR and gray, with
    and without the gate and the margin, at radius 1, 2 and 3; the sharp own frame; too few pairs; gained neighbours with the gain on and off; a
    fold pair through the occlusion test; a zoomed window; one source; the 2 x 2 dense case -- against the golden fixture, and against the
    public calls made one after another; one source alone is the window render; every tau = 0 is the own render"""
    import torch

    g = np.load(GOLDEN)
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in cases.all_cases(oracle.pose_table):
            n = case["name"] + "/"
            want = dict(image=g[n + "image"], mask=g[n + "mask"], weight=g[n + "weight"], counts=g[n + "counts"].tolist())
            got = _frame(torch, s, case)
            _same(got, want, n)
            assert np.array_equal(got["sharps"], g[n + "sharps"]), n
            taus = [rsdsfm.deblur_tau(T, cases.abi_margin(case), case["min_pairs"]) for T in got["sharps"]]
            assert taus == g[n + "taus"].tolist(), n
            s.set_occlusion_search(case["search"])
            parts, ref = _parts(torch, s, case)
            s.set_occlusion_search(0)
            _same(parts, want, n + " parts")
            if not any(taus):
                assert np.array_equal(want["image"], ref["image"]) and np.array_equal(want["mask"], ref["mask"])
            rows, cols = case["depths"][0].shape
            nsrc = len(cases.sources_and_poses(case)[0])
            assert rsdsfm.deblur_launches(rows, cols, nsrc) == nsrc * rsdsfm.stabilize_window_launches(rows, cols) + (1 if nsrc == 1 else 3 * (nsrc - 1))
        case = cases.all_cases(oracle.pose_table)[0]
        want = cases.run_spec(case)
        for with_weight, with_counts, with_records in ((False, True, True), (True, False, False)):
            _same(_frame(torch, s, case, with_weight=with_weight, with_counts=with_counts, with_records=with_records), want, "optional outputs", with_weight, with_counts)


def test_frame_argument_errors(oracle, rsdsfm):
    """a refused frame call enqueues nothing: the outputs keep their guard bytes"""
    import torch

    case = [c for c in cases.all_cases(oracle.pose_table) if c["name"] == "gained"][0]
    rows, cols = case["depths"][0].shape
    d = _clip(torch, case)
    src, M, m = cases.sources_and_poses(case)
    outs = _Outs(case["frames"][0].shape, (rows, cols))
    d_T = fresh((2, 4), np.uint64, 8, 16, _dev())
    torch.cuda.synchronize()
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    with rsdsfm.Solver(0) as s:
        def call(images=pick("frames"), maps=pick("maps"), M=M, m=m, o=outs.image.ptr, k=outs.mask.ptr, w=outs.weight.ptr, cnt_=outs.counts.ptr, T=d_T.ptr, ch=3, **kw):
            return s.deblur_frame_dev(images, ch, maps, pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, o, k, w, cnt_, T, **kw)

        bad_M = M.copy()
        bad_M[1, 0, 0] = np.nan
        params = rsdsfm.DeblurParams()
        params.struct_bytes = 48
        bads = (dict(images=[0] + pick("frames")[1:]), dict(maps=pick("maps")[:2] + [0]), dict(images=[]),
                dict(images=pick("frames") * 3, maps=pick("maps") * 3, M=np.tile(M, (3, 1, 1)), m=np.tile(m, (3, 1))),  # nine sources
                dict(M=bad_M), dict(o=0), dict(k=0), dict(o=outs.mask.ptr), dict(w=outs.image.ptr), dict(o=outs.image.ptr + 1), dict(cnt_=outs.counts.ptr + 4),
                dict(T=d_T.ptr + 4), dict(T=outs.counts.ptr), dict(o=pick("frames")[2]), dict(ch=2), dict(strength=256), dict(strength=-1), dict(margin=65), dict(margin=-2),
                dict(min_pairs=-1), dict(min_overlap=-1), dict(occlusion=2), dict(occlusion=True, occlusion_tol_q16=65537), dict(window=(0, 0, rows + 1, cols)),
                dict(window=(1, 1, 0, 4)), dict(iterations=17), dict(params=params))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        assert outs.untouched() and d_T.unchanged()
        call(**_frame_kw(case))
        s.synchronize()
        want = cases.run_spec(case)
        _same(outs.collect(), want)
        assert np.array_equal(d_T.get(), want["sharps"])


# ---------------------------------------------------------------------------------------------------
# the clip call
# ---------------------------------------------------------------------------------------------------
def _video(torch, s, case, want_counts=True, want_taus=True, with_weights=True):
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    ns = len(case["depths"])
    d = _clip(torch, case)
    outs = [_Outs(case["frames"][0].shape, (rows, cols)) for _ in range(ns)]
    torch.cuda.synchronize()
    ptrs = lambda a: [x.data_ptr() for x in a]
    s.set_occlusion_search(case["search"])
    r = s.deblur_video_dev(ptrs(d["frames"]), rows, cols, ch, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"], case["c_path"],
                           case["scales"], [o.image.ptr for o in outs], [o.mask.ptr for o in outs], [o.weight.ptr for o in outs] if with_weights else None,
                           want_counts=want_counts, want_taus=want_taus, radius=case["radius"], **_frame_kw(case))
    s.synchronize()
    s.set_occlusion_search(0)
    assert set(r) == ({"counts"} if want_counts else set()) | ({"taus"} if want_taus else set())
    got = []
    for q, o in enumerate(outs):
        one = o.collect(with_weights, False)
        one["counts"] = r["counts"][q].tolist() if want_counts else None
        one["taus"] = r["taus"][q].tolist() if want_taus else None
        got.append(one)
    return got, d


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_clip_call_equals_the_frame_calls(oracle, rsdsfm, arith):
    """five sources at radius 2 and 3 (the first and last frames with one-sided neighbours), three at radius 1, through the occlusion test, and
    one source alone: every frame of the clip call is the frame call's, which is the definition's, with its counts and its taus in the
    neighbours' order, -1 behind them; with only one of the two host arrays, and with neither (the call then only enqueues)"""
    import torch

    every = {c["name"]: c for c in cases.all_cases(oracle.pose_table)}
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in (every["blurred-own-bgr-0"], every["first-frame-radius-3"], every["gained"], every["sharp-own-gray-1"], every["one-source"], every["fold-visible"]):
            got, d = _video(torch, s, case)
            ns = len(case["depths"])
            for q in range(ns):
                want = cases.run_spec(case, q)
                _same(got[q], want, (case["name"], q))
                assert got[q]["taus"] == want["taus"] + [-1] * (6 - len(want["taus"])), (case["name"], q)
                _same(_frame(torch, s, case, d, q), want, (case["name"], q, "frame"))
            if ns == 5:
                assert [len(cases.sources_and_poses(case, q)[0]) for q in range(5)] == ([3, 4, 5, 4, 3] if case["radius"] == 2 else [4, 5, 5, 5, 4])
        case = every["blurred-own-bgr-0"]
        wants = [cases.run_spec(case, q) for q in range(5)]
        assert [w["taus"] for w in wants] == [[0, 0], [0, 0, 0], [32, 32, 32, 32], [0, 0, 0], [0, 0]]  # only frame 2 is blurred, and it gives nothing
        for want_counts, want_taus, with_weights in ((False, False, False), (True, False, True), (False, True, False)):
            got, _ = _video(torch, s, case, want_counts, want_taus, with_weights)
            for q in range(5):
                _same(got[q], wants[q], q, weight=with_weights, counts=want_counts)
                assert not want_taus or got[q]["taus"] == wants[q]["taus"] + [-1] * (6 - len(wants[q]["taus"]))
        # a refused clip call enqueues nothing
        rows, cols = case["depths"][0].shape
        d = _clip(torch, case)
        outs = [_Outs(case["frames"][0].shape, (rows, cols)) for _ in range(5)]
        torch.cuda.synchronize()
        ptrs = lambda a: [x.data_ptr() for x in a]
        bad_scales = case["scales"].copy()
        bad_scales[4] = 0.0

        def call(scales=case["scales"], o=None, **kw):
            return s.deblur_video_dev(ptrs(d["frames"]), rows, cols, 3, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"],
                                      case["c_path"], scales, o or [x.image.ptr for x in outs], [x.mask.ptr for x in outs], None, **kw)

        for bad in (dict(scales=bad_scales), dict(radius=4), dict(radius=-1), dict(strength=300), dict(margin=65), dict(min_pairs=-1), dict(o=[outs[0].image.ptr] * 4 + [0]),
                    dict(o=[outs[0].image.ptr] * 4 + [d["frames"][1].data_ptr()])):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        assert all(o.untouched() for o in outs)


# ---------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------
def test_evaluate_real_sequence_with_deblur(rsdsfm, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, deblur=True, K or (K, strength)) adds exactly deblurred, deblur_counts and deblur_taus and the
    files deblurred_<p>.png and deblur.csv, and frame 0 is the frame call's on the clip's own outputs; without the keyword every key and file is
    what it was"""
    import torch

    from test_gpu_stabilize_search import TRIALS, plain_clip

    frames, rows, cols, K, gamma, seeds, _ = plain_clip(rsdsfm)
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
    n = len(frames) - 1
    dev = _dev()
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, deblur=(1, 30), out_dir=str(tmp_path / "with"), **kw)
        plain = ev(s, frames, out_dir=str(tmp_path / "without"), **kw)
        default = ev(s, frames, deblur=True, **kw)
        ps, o = out["path_smoothed"], out["pairs"]
        src, _, M0, m0, _, _ = rsdsfm.retime_poses(out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], 0.0, nsources=n)
        nb, _, Mn, mn = rsdsfm.neighbour_poses(out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], 0, 1)
        order = list(src) + list(nb)
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_f, d_z = [tt(frames[q]) for q in order], [tt(np.asarray(o[q]["depth_map"]).T) for q in order]
        d_R, d_t = [tt(np.asarray(o[q]["R"]).reshape(-1, 9)) for q in order], [tt(o[q]["t"]) for q in order]
        outs = _Outs(frames[0].shape, (rows, cols))
        d_T = fresh((len(order) - 1, 4), np.uint64, 8, 16, dev)
        torch.cuda.synchronize()
        ptrs = lambda a: [x.data_ptr() for x in a]
        s.deblur_frame_dev(ptrs(d_f), 3, ptrs(d_z), ptrs(d_R), ptrs(d_t), K, rows, cols, np.concatenate([M0, Mn]), np.concatenate([m0, mn]), *outs.ptrs(), d_T.ptr, strength=30)
        s.synchronize()
        one = outs.collect()
        taus0 = [rsdsfm.deblur_tau(T) for T in d_T.get()]
    new = {"deblurred", "deblur_counts", "deblur_taus"}
    assert set(out) == set(plain) | new == set(default)
    assert len(out["deblurred"]) == n and out["deblur_counts"].shape == (n, 3) and out["deblur_taus"].shape == (n, 6) and default["deblur_taus"].shape == (n, 6)
    assert np.array_equal(out["deblurred"][0], one["image"]) and out["deblur_counts"][0].tolist() == one["counts"]
    assert out["deblur_taus"][0].tolist() == taus0 + [-1] * (6 - len(taus0))
    for p in range(n):
        assert out["deblurred"][p].shape == frames[0].shape and out["deblur_counts"][p].sum() == rows * cols
        listed = min(p, 1) + min(n - 1 - p, 1)
        assert (out["deblur_taus"][p][:listed] >= 0).all() and (out["deblur_taus"][p][:listed] <= 32).all() and (out["deblur_taus"][p][listed:] == -1).all()
    for k in plain:
        if k not in ("pairs", "path_smoothed", "links"):
            assert np.asarray(out[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    with_files, without_files = set(os.listdir(str(tmp_path / "with"))), set(os.listdir(str(tmp_path / "without")))
    assert with_files == without_files | {"deblurred_%d.png" % p for p in range(n)} | {"deblur.csv"}
    lines = open(str(tmp_path / "with" / "deblur.csv")).read().split()
    assert lines[0] == "pair,unset,own_only,transferred,tau_0,tau_1,tau_2,tau_3,tau_4,tau_5" and len(lines) == 1 + n
    assert lines[1].split(",") == ["0"] + [str(int(x)) for x in out["deblur_counts"][0]] + [str(int(x)) for x in out["deblur_taus"][0]]
