"""Inputs of the tests of the sharpness transfer per scanline band (tests/test_deblur_bands_cpu.py, tests/test_gpu_deblur_bands.py) and of its
golden fixture (tests/golden/make_golden_deblur_bands.py): the shapes and band heights at which the kernels can go wrong, references whose
lower rows are box-blurred (so that the band taus differ down the frame), the scene the stage is for, and the shift clip with its own frame
blurred in its lower rows only, for the frame and the clip call.  tests/deblur_cases.py's inputs are reused as they are."""
import numpy as np

import deblur_bands_spec_numpy as bands
import deblur_cases as cases
import deblur_spec_numpy as spec

# (rows, cols, band_rows): 4 bands, the last of 2 rows, cols % 4 != 0, two tile columns feeding one record; a last band of one row; a tile row
# whose 16 rows straddle a band centre (H = 32: centres 16, 48, 80; H = 48: centres 24, 72); one band
SHAPES = [(50, 70, 16), (33, 66, 16), (96, 130, 32), (96, 130, 48), (40, 64, 48)]
MIN_PAIRS = 64  # small enough for a band of 16 rows


def half_widths(rows, edge, width=cases.BLUR):
    """a box width per row: 1 above row `edge`, `width` from it on"""
    return np.where(np.arange(rows) < edge, 1, width)


def accumulate_case(rows, cols, band_rows, channels, nlayers=3, seed=0):
    """a reference whose rows from rows // 3 on are blurred, nlayers layers drawn around the SHARP reference, overlap records that give a gain on
    every second layer -> dict(ref, rmask, layers, records, band_rows, kw: the C ABI's words of the knobs)"""
    sharp, rmask = cases.reference(rows, cols, channels, seed)
    ref = bands.box_blur_rows(sharp, half_widths(rows, rows // 3))
    ls = cases.layers(sharp, rows, cols, channels, nlayers, seed)
    recs = [list(cases.records(channels).values())[(seed + j) % 5] if j % 2 else None for j in range(nlayers)]
    return dict(name="%dx%d-h%d-%s-%d" % (rows, cols, band_rows, "bgr" if channels == 3 else "gray", seed), ref=ref, rmask=rmask, layers=ls, records=recs,
                band_rows=band_rows, kw=dict(min_pairs=MIN_PAIRS, strength=40, margin=2))


def accumulate_cases():
    return [accumulate_case(r, c, h, ch, seed=i) for i, (r, c, h) in enumerate(SHAPES) for ch in (1, 3)]


def spec_kw(kw):
    """the ABI's words of a call as the definition's values"""
    return dict(min_overlap=kw.get("min_overlap", 0) or spec.MIN_OVERLAP_DEFAULT, gain_mode=kw.get("gain_mode", 0), strength=kw.get("strength", 0) or spec.STRENGTH_DEFAULT,
                margin=spec.margin_value(kw.get("margin", 0)), min_pairs=kw.get("min_pairs", 0) or spec.MIN_PAIRS_DEFAULT, gate_mode=kw.get("gate_mode", 0))


def run_accumulate(case, band_rows=None):
    return bands.deblur(case["ref"], case["rmask"], case["layers"], band_rows or case["band_rows"], case["records"], None, **spec_kw(case["kw"]))


def purpose_scene(channels, rows=96, cols=130, noise=6, neighbours=4, seed=0):
    """what the stage is for: a texture drawn from 32 .. 223 (noise of +-6 never clips), the own frame's lower half box-blurred over 5 columns,
    four sharp neighbours under identity registration, i.i.d. noise in [-noise, noise] on every frame, every mask full
    -> dict(clean, ref, rmask, layers, edge)"""
    rng = np.random.default_rng(4200 + 10 * seed + channels)
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    # patches of 2 x 3 pixels: a texture with edges a 5-column box visibly smears
    coarse = rng.integers(32, 224, size=(-(-rows // 2), -(-cols // 3)) + shape[2:])
    clean = np.repeat(np.repeat(coarse, 2, axis=0), 3, axis=1)[:rows, :cols].astype(np.uint8)
    edge = rows // 2
    noisy = lambda a: (a.astype(np.int64) + rng.integers(-noise, noise + 1, size=a.shape)).astype(np.uint8)
    ref = noisy(bands.box_blur_rows(clean, half_widths(rows, edge)))
    full = np.ones((rows, cols), dtype=np.uint8)
    return dict(clean=clean, ref=ref, rmask=full, layers=[(noisy(clean), full) for _ in range(neighbours)], edge=edge)


def band_blur_clip(channels=3, seed=0, band_rows=16, edge=12, **kw):
    """deblur_cases.blur_clip's scene (five frames of 24 x 40) with frame q = 2 blurred in its rows from `edge` on only: two bands at
    band_rows = 16, the last of 8 rows.  A frame case with case["band_rows"]"""
    base = cases.blur_clip("blurred-own", seed, channels, noise=0, width=1, name="band-%s-%d" % ("bgr" if channels == 3 else "gray", seed), **kw)
    rng = np.random.default_rng(9100 + seed)
    frames = list(base["clean"])
    frames[base["q"]] = bands.box_blur_rows(frames[base["q"]], half_widths(frames[0].shape[0], edge))
    frames = [(fr.astype(np.int64) + rng.integers(-6, 7, size=fr.shape)).astype(np.uint8) for fr in frames]
    return dict(base, frames=frames, band_rows=band_rows)


def frame_cases():
    # two bands, BGR (the blur's edge inside the first band) and gray (the edge on the band border: the first band transfers nothing); one band
    return [band_blur_clip(3, 0), band_blur_clip(1, 1, edge=16), band_blur_clip(3, 2, band_rows=32)]


def run_frame(case, q=None):
    """the banded definition on frame q of a frame case -> deblur_bands_spec_numpy.deblur_frame's dict plus sources"""
    src, M, m = cases.sources_and_poses(case, q)
    pick = lambda k: [case[k][n] for n in src]
    r = bands.deblur_frame(pick("frames"), pick("depths"), pick("Rs"), pick("ts"), case["K"], M, m, case["band_rows"], case["window"], case["strength"], case["margin"],
                           case["min_pairs"], case["gate_mode"], case["min_overlap"], case["gain_mode"], occlusion=case["occlusion"], search_on=case["search"],
                           tol_q16=case["tol_q16"], mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    return dict(r, sources=src)
