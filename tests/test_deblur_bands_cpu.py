"""GPU-free tests of the sharpness transfer per scanline band (include/rsdsfm_deblur.h, "per scanline band"): the definition
(tests/deblur_bands_spec_numpy.py) against a second, loop-form transcription and against its golden fixture; its consequences (the band records
sum to the whole-frame record; one band is the unbanded definition; every band tau 0 is the own frame; the order of the layers); the row taus'
shape and the library's two host functions against the definition; what the stage is for on a frame whose lower half is blurred; the
library's surface and the synthetic per-row blur."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import deblur_bands_cases as bcases  # noqa: E402
import deblur_bands_spec_numpy as bands  # noqa: E402
import deblur_cases as cases  # noqa: E402
import deblur_spec_numpy as spec  # noqa: E402
import denoise_spec_numpy as dn  # noqa: E402
from make_golden_deblur_bands import digest, results  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_deblur_bands_v1.npz")
HEADER_TEXT = open(os.path.join(ROOT, "include", "rsdsfm_deblur.h")).read()
NEW_SYMBOLS = {"rsdsfm_deblur_band_sharpness_dev", "rsdsfm_deblur_band_taus", "rsdsfm_deblur_row_taus", "rsdsfm_deblur_band_accumulate_dev",
               "rsdsfm_deblur_video_banded_dev"}
ERR_INVALID = -1


# ---------------------------------------------------------------------------------------------------
# the definition, a second time: loops over pixels, Python integers
# ---------------------------------------------------------------------------------------------------
def _loop_row_tau(taus, H, y):
    nb = len(taus)
    if y < H // 2:
        return taus[0]
    if y >= (nb - 1) * H + H // 2:
        return taus[nb - 1]
    b = (y - H // 2) // H
    f = (y - H // 2) - b * H
    return (taus[b] * (H - f) + taus[b + 1] * f + H // 2) // H


def _loop_deblur(ref, rmask, layers, records, H, min_overlap, gain_mode, strength, margin, min_pairs, gate_mode):
    rows, cols = rmask.shape
    R = ref.reshape(rows, cols, -1)
    ch = R.shape[2]
    nb = -(-rows // H)
    cells = [[[16 * int(b) for b in R[y, x]] + [16] if rmask[y, x] else [0] * (ch + 1) for x in range(cols)] for y in range(rows)]
    all_records, all_taus = [], []
    for j, (limg, lmask) in enumerate(layers):
        L = limg.reshape(rows, cols, -1)
        G = dn.gains(records[j] if records else None, ch, min_overlap, gain_mode)
        k = [[[min(255, (int(G[c]) * int(L[y, x, c]) + 32768) >> 16) for c in range(ch)] for x in range(cols)] for y in range(rows)]
        v = [[bool(rmask[y, x]) and bool(lmask[y, x]) for x in range(cols)] for y in range(rows)]
        yr = [[sum(int(b) for b in R[y, x]) for x in range(cols)] for y in range(rows)]
        yl = [[sum(k[y][x]) for x in range(cols)] for y in range(rows)]
        T = [[0, 0, 0, 0] for _ in range(nb)]
        for y in range(rows):
            for x in range(cols):
                for qy, qx in ((y, x + 1), (y + 1, x)):
                    if v[y][x] and qy < rows and qx < cols and v[qy][qx]:
                        T[y // H][0] += 1
                        T[y // H][1] += (yr[y][x] - yr[qy][qx]) ** 2
                        T[y // H][2] += (yl[y][x] - yl[qy][qx]) ** 2
        taus = [0 if p < min_pairs or 16 * al <= (16 + margin) * ar else min(32, (16 * (al - ar)) // max(ar, 1)) for p, ar, al, _ in T]
        all_records.append(T)
        all_taus.append(taus)
        for y in range(rows):
            t = _loop_row_tau(taus, H, y)
            for x in range(cols):
                if not v[y][x]:
                    continue
                d = n = 0
                for py in range(max(y - 1, 0), min(y + 2, rows)):
                    for px in range(max(x - 1, 0), min(x + 2, cols)):
                        if v[py][px]:
                            d += yr[py][px] - yl[py][px]
                            n += ch
                w = 16 if gate_mode == 1 else 16 - min(16, (16 * abs(d)) // (strength * n))
                u = (w * t + 8) >> 4
                for c in range(ch):
                    cells[y][x][c] += u * k[y][x][c]
                cells[y][x][ch] += u
    image = np.zeros((rows, cols, ch), dtype=np.uint8)
    weight = np.zeros((rows, cols), dtype=np.uint8)
    for y in range(rows):
        for x in range(cols):
            n = cells[y][x][ch]
            weight[y, x] = n
            if n:
                image[y, x] = [(2 * s + n) // (2 * n) for s in cells[y][x][:ch]]
    counts = [int((weight == 0).sum()), int((weight == 16).sum()), int((weight > 16).sum())]
    return dict(image=image.reshape(ref.shape), mask=(weight > 0).astype(np.uint8), weight=weight, counts=counts, band_records=all_records, band_taus=all_taus)


@pytest.mark.parametrize("channels", [1, 3])
def test_spec_equals_a_loop_form_transcription(channels):
    """random cases of 17 .. 40 rows (two or three bands of 16, the last one short) by 2 .. 9 columns: one to three layers around a reference whose
    lower rows are blurred, masks with holes, overlap records that give a gain, both gate modes, margins 0 .. 64"""
    rng = np.random.default_rng(177 + channels)
    seen = set()
    for trial in range(10):
        rows, cols = int(rng.integers(17, 41)), int(rng.integers(2, 10))
        sharp, rmask = cases.reference(rows, cols, channels, seed=trial)
        ref = bands.box_blur_rows(sharp, bcases.half_widths(rows, int(rng.integers(0, rows)), 3))
        ls = cases.layers(sharp, rows, cols, channels, 1 + trial % 3, seed=trial)
        recs = [list(cases.records(channels).values())[(trial + j) % 5] for j in range(len(ls))] if trial % 2 else None
        kw = dict(min_overlap=int(rng.choice([1, 1024, 6000])), gain_mode=int(trial % 5 == 0), strength=int(rng.choice([1, 7, 24, 255])), margin=int(rng.choice([0, 4, 64])),
                  min_pairs=int(rng.choice([1, 30])), gate_mode=int(trial % 4 == 3))
        want = _loop_deblur(ref, rmask, ls, recs, 16, **kw)
        got = bands.deblur(ref, rmask, ls, 16, recs, None, **kw)
        for k in ("image", "mask", "weight"):
            assert np.array_equal(got[k], want[k]), (trial, k)
        assert got["counts"] == want["counts"] and got["band_taus"] == want["band_taus"] and got["band_records"].tolist() == want["band_records"], trial
        seen |= {t for taus in want["band_taus"] for t in taus}
    assert 0 in seen and 32 in seen and len(seen) >= 4, seen


def test_spec_equals_the_golden_fixture():
    g = np.load(GOLDEN)
    done = results()
    assert {k.split("/")[0] for k in g.files} == {c["name"] for c, _ in done}
    taus = set()
    for case, r in done:
        n = case["name"] + "/"
        assert digest(case) == int(g[n + "digest"]), n
        for k in ("image", "mask", "weight", "band_records"):
            assert np.array_equal(r[k], g[n + k]), n + k
        assert r["counts"] == g[n + "counts"].tolist() and r["band_taus"] == g[n + "band_taus"].tolist(), n
        taus |= {t for ts in r["band_taus"] for t in ts}
        if len(r["band_taus"][0]) > 1:
            assert any(len(set(ts)) > 1 for ts in r["band_taus"]), n  # the bands differ: the fixture is about them
    assert 0 in taus and 32 in taus and len(taus) >= 6, taus


# ---------------------------------------------------------------------------------------------------
# consequences
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("band_rows", [16, 32, 48])
def test_the_band_records_sum_to_the_whole_frame_record(channels, band_rows):
    for seed, (rows, cols) in enumerate([(50, 70), (33, 9), (96, 21), (17, 5)]):
        sharp, rmask = cases.reference(rows, cols, channels, seed)
        for j, (limg, lmask) in enumerate(cases.layers(sharp, rows, cols, channels, 2, seed)):
            rec = list(cases.records(channels).values())[(seed + j) % 5] if j else None
            T = bands.band_sharpness(sharp, rmask, limg, lmask, band_rows, rec)
            assert T.shape == (-(-rows // band_rows), 4)
            assert T.sum(axis=0).tolist() == spec.sharpness(sharp, rmask, limg, lmask, rec).tolist(), (rows, cols, j)


@pytest.mark.parametrize("channels", [1, 3])
def test_one_band_is_the_unbanded_definition(channels):
    for case in (bcases.accumulate_case(40, 64, 48, channels), bcases.accumulate_case(33, 21, 64, channels, seed=1), bcases.accumulate_case(16, 9, 16, channels, seed=2)):
        kw = bcases.spec_kw(case["kw"])
        got = bcases.run_accumulate(case)
        want = spec.deblur(case["ref"], case["rmask"], case["layers"], case["records"], None, **kw)
        assert got["band_records"][:, 0].tolist() == want["sharps"].tolist() and [t[0] for t in got["band_taus"]] == want["taus"]
        for k in ("image", "mask", "weight"):
            assert np.array_equal(got[k], want[k]), k
        assert got["counts"] == want["counts"] and all(np.array_equal(a, b) for a, b in zip(got["cells"], want["cells"]))


@pytest.mark.parametrize("channels", [1, 3])
def test_every_band_tau_zero_is_the_own_frame(channels):
    case = bcases.accumulate_case(50, 70, 16, channels)
    own = spec.deblur(case["ref"], case["rmask"], [])
    for kw in (dict(min_pairs=10 ** 9), dict(margin=64, min_pairs=1)):
        zero = [np.array([[5000, 1000, 1000, 0]] * 4, dtype=np.uint64)] * 3 if "margin" in kw else None  # records at "equal": below every margin
        got = bands.deblur(case["ref"], case["rmask"], case["layers"], 16, case["records"], zero, **dict(bcases.spec_kw(case["kw"]), **kw))
        assert all(t == [0, 0, 0, 0] for t in got["band_taus"])
        for k in ("image", "mask", "weight"):
            assert np.array_equal(got[k], own[k]), k
        assert got["counts"] == own["counts"]
    # a row both of whose surrounding bands have tau 0 keeps its bytes; the others may change
    recs = [np.array([[5000, 1000, 1000, 0], [5000, 1000, 1000, 0], [5000, 1000, 3000, 0], [5000, 1000, 3000, 0]], dtype=np.uint64)] * 3
    got = bands.deblur(case["ref"], case["rmask"], case["layers"], 16, case["records"], recs, **bcases.spec_kw(case["kw"]))
    assert got["band_taus"][0] == [0, 0, 32, 32] and (got["row_taus"][0][:25] == 0).all() and (got["row_taus"][0][25:] > 0).all()
    assert np.array_equal(got["image"][:25], own["image"][:25]) and np.array_equal(got["weight"][:25], own["weight"][:25])
    assert not np.array_equal(got["image"][25:], own["image"][25:])


def test_no_order_of_the_layers_changes_a_byte():
    case = bcases.accumulate_case(50, 70, 16, 3)
    base = bcases.run_accumulate(case)
    assert len({tuple(t) for t in base["band_taus"]}) >= 1 and any(any(t) for t in base["band_taus"])
    for order in itertools.permutations(range(3)):
        got = bands.deblur(case["ref"], case["rmask"], [case["layers"][j] for j in order], 16, [case["records"][j] for j in order], None, **bcases.spec_kw(case["kw"]))
        for k in ("image", "mask", "weight"):
            assert np.array_equal(got[k], base[k]), (order, k)
        assert got["counts"] == base["counts"]


# ---------------------------------------------------------------------------------------------------
# the row taus and the host functions
# ---------------------------------------------------------------------------------------------------
def test_the_row_taus_end_flat_hit_the_centres_and_are_monotone_between_them(rsdsfm):
    rng = np.random.default_rng(5)
    for rows, H in ((50, 16), (33, 16), (96, 32), (96, 48), (40, 48), (130, 16), (1040, 32)):
        nb = bands.nbands(rows, H)
        for trial in range(20):
            taus = rng.integers(0, 33, nb) if trial else np.array([0, 32] * nb)[:nb]
            r = bands.row_taus(taus, H, rows)
            assert r.shape == (rows,) and r.min() >= 0 and r.max() <= 32
            assert (r[:H // 2] == taus[0]).all() and (r[(nb - 1) * H + H // 2:] == taus[-1]).all()
            for b in range(nb):
                c = b * H + H // 2
                if c < rows:
                    assert r[c] == taus[b], (rows, H, b)
                if b + 1 < nb:
                    seg = r[c:min(c + H + 1, rows)]
                    assert (np.diff(seg) >= 0).all() if taus[b + 1] >= taus[b] else (np.diff(seg) <= 0).all(), (rows, H, b)
            assert [_loop_row_tau(taus.tolist(), H, y) for y in range(rows)] == r.tolist()
            assert rsdsfm.deblur_row_taus(taus, H, rows).tolist() == r.tolist(), (rows, H, taus)


def test_the_host_functions_equal_the_definition_on_every_record_case(rsdsfm):
    recs = cases.sharp_records()
    T = np.array([r for r, _ in recs.values()], dtype=np.uint64)
    assert rsdsfm.deblur_band_taus(T).tolist() == [t for _, t in recs.values()] == bands.band_taus(T)
    for margin, min_pairs in ((-1, 1), (64, 5000), (1, 1024), (0, 0)):
        want = bands.band_taus(T, spec.margin_value(margin), min_pairs or spec.MIN_PAIRS_DEFAULT)
        got = rsdsfm.deblur_band_taus(T, margin, min_pairs)
        assert got.tolist() == want == [rsdsfm.deblur_tau(t, margin, min_pairs) for t in T]
        nb = len(want)
        assert rsdsfm.deblur_row_taus(got, 16, 16 * nb - 3).tolist() == bands.row_taus(want, 16, 16 * nb - 3).tolist()
    lib = rsdsfm.load_library()
    out = (ctypes.c_int32 * 80)()
    p64 = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    i32 = np.zeros(80, dtype=np.int32)
    for bad in ((None, 1, 0, 0, out), (p64(T), 0, 0, 0, out), (p64(T), 65, 0, 0, out), (p64(T), 2, 65, 0, out), (p64(T), 2, 0, -1, out), (p64(T), 2, 0, 0, None)):
        assert lib.rsdsfm_deblur_band_taus(bad[0], ctypes.c_int32(bad[1]), ctypes.c_int32(bad[2]), ctypes.c_int64(bad[3]), bad[4]) == ERR_INVALID, bad[1:4]
    big = np.full(80, 33, dtype=np.int32)
    rows_out = (ctypes.c_int32 * 2048)()
    for taus, nb, H, rows in ((None, 2, 16, 32), (i32, 2, 8, 16), (i32, 2, 24, 48), (i32, 2, -16, 32), (i32, 1, 16400, 100), (i32, 3, 16, 32), (i32, 65, 16, 1040), (i32, 1, 16, 1),
                              (big, 2, 16, 32)):
        ptr = None if taus is None else taus.ctypes.data_as(ctypes.c_void_p)
        assert lib.rsdsfm_deblur_row_taus(ptr, ctypes.c_int32(nb), ctypes.c_int32(H), ctypes.c_int32(rows), rows_out) == ERR_INVALID, (nb, H, rows)
    assert lib.rsdsfm_deblur_row_taus(i32.ctypes.data_as(ctypes.c_void_p), ctypes.c_int32(2), ctypes.c_int32(16), ctypes.c_int32(32), None) == ERR_INVALID


# ---------------------------------------------------------------------------------------------------
# what it is for
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
def test_a_half_blurred_frame_keeps_its_sharp_half_and_gains_more_in_its_blurred_half(channels):
    """96 x 130, the lower half box-blurred over 5 columns, noise +-6, four sharp neighbours, min_pairs 64, H = 16: at least H above the blur's
    edge the banded output is the own frame's bytes; at least H below it the error against the clean frame is strictly below the global
    call's, which is strictly below the own frame's.  The ordering only; DESIGN has the ratios"""
    sc = bcases.purpose_scene(channels)
    H, edge = 16, sc["edge"]
    kw = dict(min_pairs=64)
    glob = spec.deblur(sc["ref"], sc["rmask"], sc["layers"], **kw)
    band = bands.deblur(sc["ref"], sc["rmask"], sc["layers"], H, **kw)
    print("global taus", glob["taus"], "band taus", band["band_taus"])
    assert all(0 < t < 32 for t in glob["taus"])  # over the margin, and diluted
    assert all(t[:2] == [0, 0] and min(t[3:]) > max(glob["taus"]) for t in band["band_taus"])
    assert (band["band_records"].sum(axis=1) == glob["sharps"]).all()
    above, below = slice(0, edge - H), slice(edge + H, None)
    assert np.array_equal(band["image"][above], sc["ref"][above]) and not np.array_equal(glob["image"][above], sc["ref"][above])
    err = lambda a: float(np.abs(a[below].astype(np.int64) - sc["clean"][below].astype(np.int64)).mean())
    e_own, e_glob, e_band = err(sc["ref"]), err(glob["image"]), err(band["image"])
    print("channels", channels, "error below the edge: own", e_own, "global", e_glob, e_glob / e_own, "banded", e_band, e_band / e_own)
    assert e_band < e_glob < e_own


# ---------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------
def test_header_symbols_and_params(rsdsfm):
    assert "#define RSDSFM_DEBLUR_BANDS_MAX 64" in HEADER_TEXT and "int32_t band_rows;" in HEADER_TEXT and "int32_t reserved[3];" in HEADER_TEXT
    assert "NOT here" in HEADER_TEXT and "scanline band" not in HEADER_TEXT[HEADER_TEXT.index("NOT here"):HEADER_TEXT.index("*/")]
    assert HEADER_TEXT.count("choices, not measurements") >= 3 and "linear interpolation" in HEADER_TEXT
    assert NEW_SYMBOLS <= set(rsdsfm.declared_symbols())
    for arith in ("reference", "fused"):
        lib = rsdsfm.load_library(arith=arith)
        assert all(hasattr(lib, n) for n in NEW_SYMBOLS), arith
    assert ctypes.sizeof(rsdsfm.DeblurParams) == 64 and rsdsfm.DEBLUR_BANDS_MAX == bands.BANDS_MAX
    p = rsdsfm.DeblurParams()
    assert rsdsfm.load_library().rsdsfm_deblur_params_init(ctypes.byref(p)) == 0 and p.struct_bytes == 64 and p.band_rows == 0 and list(p.reserved) == [0, 0, 0, 0]
    p.band_rows = 48
    assert list(p.reserved) == [48, 0, 0, 0] and rsdsfm.DeblurParams.band_rows.offset == 48
    assert rsdsfm.deblur_default_params()["band_rows"] == 0
    for name in ("deblur_band_sharpness_dev", "deblur_band_sharpness", "deblur_band_accumulate_dev", "deblur_band_accumulate"):
        assert callable(getattr(rsdsfm.Solver, name))


def test_refusals_without_a_context(rsdsfm):
    lib = rsdsfm.load_library()
    z = ctypes.c_void_p(0)
    i, q = ctypes.c_int32, ctypes.c_int64
    assert lib.rsdsfm_deblur_band_sharpness_dev(None, z, z, z, z, i(3), i(32), i(32), z, q(0), i(0), i(16), z) == ERR_INVALID
    assert lib.rsdsfm_deblur_band_accumulate_dev(None, z, z, z, z, i(3), i(32), i(32), z, q(0), i(0), i(0), z, i(16), i(0), q(0), i(0), z, i(1), i(1), z, z, z, z) == ERR_INVALID
    d = ctypes.c_double(1.0)
    assert lib.rsdsfm_deblur_video_banded_dev(None, z, i(2), i(32), i(32), i(3), d, d, d, d, z, z, z, z, z, z, z, z, 0, 0, i(0), z, z, z, z, z, z, z, z) == ERR_INVALID


def test_render_sequence_blurs_a_frame_row_by_row(rsdsfm):
    synth = rsdsfm.synth
    rows, cols = 32, 48
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = synth.default_motion()
    plain, flow0, mask0 = synth.render_sequence(3, rows, cols, K, v, w, k, seed=3)
    widths = bcases.half_widths(rows, 20)
    got, flow1, mask1 = synth.render_sequence(3, rows, cols, K, v, w, k, seed=3, blur=[1, widths, 3])
    assert np.array_equal(flow0, flow1) and np.array_equal(mask0, mask1)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], bands.box_blur_rows(plain[1], widths)) and np.array_equal(got[2], spec.box_blur(plain[2], 3))
    assert np.array_equal(got[1][:20], plain[1][:20]) and not np.array_equal(got[1][20:], plain[1][20:])
    # a scalar entry, and an entry of equal widths, are the frame-wide blur; all 1 is the plain clip
    same = synth.render_sequence(3, rows, cols, K, v, w, k, seed=3, blur=[1, np.full(rows, 5), 3])[0]
    assert np.array_equal(same, synth.render_sequence(3, rows, cols, K, v, w, k, seed=3, blur=[1, 5, 3])[0])
    assert np.array_equal(synth.render_sequence(3, rows, cols, K, v, w, k, seed=3, blur=[1, np.ones(rows, dtype=int), 1])[0], plain)
    for bad in ([1, widths[:-1], 1], [1, np.full(rows, 4), 1], [1, np.zeros(rows, dtype=int), 1], [1, widths]):
        with pytest.raises(ValueError):
            synth.render_sequence(3, rows, cols, K, v, w, k, seed=3, blur=bad)
