"""Executable definition of the mover removal (include/rsdsfm_erase.h): the clean plate's raw flag (tests/plate_spec_numpy.py: 0 unset, 1 static,
2 moving, 3 undecided) turned into a MATTE -- speckle removed, grown, feathered -- and the plate put under that matte while every other pixel keeps
the own frame's bytes: the frame without what walked through it.  The reference has no counterpart (main.cc:380-523 solves pairs one by one and
never relates them); this file is the definition and the kernels (csrc/erase_kernels.hip) and host functions (csrc/erase_host.hip) reproduce it
bit for bit.  The plate, the renders, the records and the gains are tests/plate_spec_numpy.py's, tests/stabilize_crop_spec_numpy.py's,
tests/retime_spec_numpy.py's and tests/stabilize_blend_spec_numpy.py's, imported and unchanged.

Integers only.  open o 0 .. 3 (default 2), grow g 0 .. 8 (default 2), feather T 1 .. 16 (default 4): choices, not measurements.

matte       seed     s(p) = F(p) == 2, or F(p) == 3 with include_undecided; every other byte value (values above 3 too) is no seed
            core     core(p) = s(p') for every p' of the (2 o + 1)^2 window about p INSIDE the frame (outside the frame nothing vetoes)
            distance d(p) = the chessboard distance from p to the nearest core pixel, capped at C = o + g + T
            matte    a(p) = clamp(C - d(p), 0, T): T within o + g of the core, one less per pixel beyond, 0 from distance C on
composite   a matte byte above T counts as T; mR, mP set iff not 0
            mR unset                  image 0, mask 0                                  counted unset
            mR set, a == 0            the bytes of R, mask 1                           counted kept
            mR set, a > 0, mP unset   the bytes of R, mask 1                           counted unresolved
            mR set, a > 0, mP set     out_c = (a P_c + (T - a) R_c + (T >> 1)) // T, mask 1; a == T (out = P exactly) counted replaced,
                                      else counted feathered
counts      [unset, kept, replaced, feathered, unresolved]
frame       plate.plate_frame (plate, its mask, the flag); the own frame through the window with id 1 on zeroed planes (the plate's own
            reference planes: the same render); the matte of the flag; the composite.

Not here: temporal smoothing of the matte across frames; filling the own frame's empty band from the plate; the matte fed into the denoise, the
super-resolution or the fill; inpainting where every source saw the mover.
"""
import numpy as np

import plate_spec_numpy as plate
import stabilize_blend_spec_numpy as blend

OPEN_DEFAULT, OPEN_MAX = 2, 3        # choices, not measurements
GROW_DEFAULT, GROW_MAX = 2, 8
FEATHER_DEFAULT, FEATHER_MAX = 4, 16
REACH_MAX = OPEN_MAX + GROW_MAX + FEATHER_MAX  # 27
COUNT_NAMES = ("unset", "kept", "replaced", "feathered", "unresolved")

_planes = blend._planes


def seeds(flag, include_undecided=0):
    F = np.asarray(flag)
    return (F == 2) | ((F == 3) if include_undecided else np.zeros(F.shape, dtype=bool))


def _shifted(plane, dy, dx, outside):
    """plane moved so that out[y, x] = plane[y + dy, x + dx], `outside` where that lies outside the frame"""
    rows, cols = plane.shape
    out = np.full(plane.shape, outside, dtype=plane.dtype)
    ys, xs = slice(max(0, -dy), min(rows, rows - dy)), slice(max(0, -dx), min(cols, cols - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[ys, xs] = plane[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return out


def core_of(seed, o):
    """the seed eroded by the (2 o + 1)^2 window, pixels outside the frame not vetoing"""
    core = np.asarray(seed, dtype=bool).copy()
    for dy in range(-o, o + 1):
        for dx in range(-o, o + 1):
            core &= _shifted(seed, dy, dx, True)
    return core


def core_distance(core, C):
    """the chessboard distance to the nearest core pixel, capped at C"""
    d = np.full(core.shape, C, dtype=np.int64)
    reach = np.asarray(core, dtype=bool)
    for k in range(C):
        if k:
            grown = reach.copy()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    grown |= _shifted(reach, dy, dx, False)
            reach = grown
        d = np.where(reach, np.minimum(d, k), d)
    return d


def matte(flag, open=OPEN_DEFAULT, grow=GROW_DEFAULT, feather=FEATHER_DEFAULT, include_undecided=0):
    """flag (rows, cols) bytes -> the matte (rows, cols) uint8, 0 .. feather"""
    o, g, T = int(open), int(grow), int(feather)
    assert 0 <= o <= OPEN_MAX and 0 <= g <= GROW_MAX and 1 <= T <= FEATHER_MAX and include_undecided in (0, 1)
    C = o + g + T
    d = core_distance(core_of(seeds(flag, include_undecided), o), C)
    return np.clip(C - d, 0, T).astype(np.uint8)


def composite(ref, ref_mask, plate_image, plate_mask, matte_plane, feather=FEATHER_DEFAULT):
    """-> dict(image, mask, counts [unset, kept, replaced, feathered, unresolved])"""
    T = int(feather)
    assert 1 <= T <= FEATHER_MAX
    gray = np.asarray(ref).ndim == 2
    R, P = _planes(ref).astype(np.int64), _planes(plate_image).astype(np.int64)
    mR, mP = np.asarray(ref_mask) != 0, np.asarray(plate_mask) != 0
    a = np.minimum(np.asarray(matte_plane).astype(np.int64), T)
    assert R.shape == P.shape and mR.shape == mP.shape == a.shape == R.shape[:2]
    mix = (a[..., None] * P + (T - a[..., None]) * R + (T >> 1)) // T
    use = mR & (a > 0) & mP
    out = np.where(use[..., None], mix, np.where(mR[..., None], R, 0)).astype(np.uint8)
    counts = [int((~mR).sum()), int((mR & (a == 0)).sum()), int((use & (a == T)).sum()), int((use & (a < T)).sum()), int((mR & (a > 0) & ~mP).sum())]
    return dict(image=out[..., 0] if gray else out, mask=mR.astype(np.uint8), counts=counts)


def erase_frame(images, depths, Rs, ts, K, M, m, window=None, open=OPEN_DEFAULT, grow=GROW_DEFAULT, feather=FEATHER_DEFAULT, include_undecided=0,
                threshold=plate.THRESHOLD_DEFAULT, min_votes=plate.MIN_VOTES_DEFAULT, min_overlap=plate.MIN_OVERLAP_DEFAULT, gain_mode=0, occlusion=0, search_on=0, tol_q16=0,
                mode=0, q5_mode=0, iterations=0):
    """the sources and poses as plate.plate_frame takes them
    -> dict(image, mask, matte, moving (the plate's flag), counts, plate (plate_frame's dict: its image, mask, ref, ...))"""
    p = plate.plate_frame(images, depths, Rs, ts, K, M, m, window, threshold, min_votes, min_overlap, gain_mode, occlusion, search_on, tol_q16, mode, q5_mode, iterations)
    ref, rmask, _ = p["ref"]  # the own frame through the window with id 1 on zeroed planes
    a = matte(p["moving"], open, grow, feather, include_undecided)
    out = composite(ref, rmask, p["image"], p["mask"], a, feather)
    return dict(out, matte=a, moving=p["moving"], plate=p)
