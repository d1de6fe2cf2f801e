"""Executable definition of the stabiliser's border fill (include/rsdsfm_stabilize_fill.h): the band of a stabilised frame that its own
frame does not cover, filled from the neighbouring frames of the clip, each rendered into the SAME virtual camera.  The reference has no
counterpart (main.cc:380-523 solves pairs one by one and never relates them); this file is the definition and the kernels
(csrc/stabilize_fill_kernels.hip, compiled with -ffp-contract=off) and host functions (csrc/stabilize_fill_host.hip) reproduce it -- the
frame call bit for bit.  tests/stabilize_spec_numpy.py, tests/rectify_dense_spec_numpy.py and tests/link_spec_numpy.py are imported and
unchanged.

All arithmetic is float64 with one rounding per operation; sums are taken in the order written.

neighbour_order        the candidates of frame q: n = q - 1, q + 1, q - 2, q + 2, ..., q - radius, q + radius -- nearer first, previous before
                       next -- of which 0 <= n <= npairs - 1 are kept (the clip's last frame has no pair, hence no depth: never a candidate).
source_id              of the neighbour at offset j = n - q: 2 |j| for j < 0, 2 |j| + 1 for j > 0.  1 is the own frame, 0 nobody.
neighbour_pose         M_{q,n} = A~_q^T A_n,  m_{q,n} = (A~_q^T (c_n - c~_q)) / S_n: a point X in the coordinates of frame n's first scanline,
                       in pair n's own unit, is M X + m in virtual camera q's.  The scales are ALWAYS read: the baseline between two frames
                       is real even when the path's translation is not smoothed (then c~ = c).  n = q is virtual_poses' business.
fill_from              cand = stabilize_frame(neighbour n seen with (M, m)); take = (mask == 0) & (cand mask == 1); where take holds, out gets
                       cand's pixel, mask 1 and source the neighbour's source id.  A candidate without one valid depth offers nothing
                       (stabilize_frame's mask is then 0 everywhere).
stabilize_filled_frame the own stabilize_frame, source = mask, then fill_from over neighbour_order: the first that offers a pixel keeps it.

Not here: blending or feathering at the seams, exposure compensation, occlusion tests between candidates (a fold of a neighbour's map fills
like any pixel), moving objects, the clip's last frame, inpainting of what nobody saw.
"""
import numpy as np

import link_spec_numpy as link  # noqa: F401  (the chain that gives A, c and the scales)
import rectify_dense_spec_numpy as dense  # noqa: F401  (stabilize_frame's stages A and C)
import stabilize_spec_numpy as stab

RADIUS_DEFAULT = 2  # neighbours on each side: a choice, not a measurement
RADIUS_MAX = 16


def source_id(j):
    """of the neighbour at offset j != 0"""
    assert j != 0
    return 2 * abs(j) + (1 if j > 0 else 0)


def neighbour_order(q, npairs, radius=RADIUS_DEFAULT):
    """-> the candidate frames of frame q, in the order they are asked"""
    assert 0 <= q <= npairs - 1 and 1 <= radius <= RADIUS_MAX
    out = []
    for d in range(1, radius + 1):
        for n in (q - d, q + d):
            if 0 <= n <= npairs - 1:
                out.append(n)
    return out


def neighbour_pose(A, c, As, cs, scales, q, n):
    """-> M (3, 3), m (3): frame n's first-scanline coordinates (pair n's unit) to virtual camera q's"""
    A, As = np.asarray(A, dtype=np.float64).reshape(-1, 3, 3), np.asarray(As, dtype=np.float64).reshape(-1, 3, 3)
    c, cs = np.asarray(c, dtype=np.float64).reshape(-1, 3), np.asarray(cs, dtype=np.float64).reshape(-1, 3)
    assert n != q
    S = np.float64(np.asarray(scales, dtype=np.float64).reshape(-1)[n])
    assert np.isfinite(S) and S > 0
    Ast = As[q].T
    return stab._mat3(Ast, A[n]), stab._matvec(Ast, c[n] - cs[q]) / S


def fill_from(out, mask, source, image_n, depth_n, R_n, t_n, K, M, m, source_id, mode=0, q5_mode=0, iterations=0):
    """one neighbour: out, mask and source are changed IN PLACE where the mask is 0 and the candidate is valid.  -> the number of pixels taken"""
    assert 2 <= source_id <= 255
    cand = stab.stabilize_frame(image_n, depth_n, R_n, t_n, K, M, m, mode=mode, q5_mode=q5_mode, iterations=iterations)
    take = (mask == 0) & (cand["mask"] == 1)
    out[take] = cand["image"][take]
    mask[take] = 1
    source[take] = source_id
    return int(take.sum())


def stabilize_filled_frame(images, depths, Rs, ts, K, A, c, As, cs, scales, q, M_own, m_own, radius=RADIUS_DEFAULT, mode=0, q5_mode=0, iterations=0):
    """frame q of a clip: images / depths / Rs / ts are indexed by frame (entries q and its candidates are read), (M_own, m_own) is
    virtual_poses' pose of q.  -> dict(image, mask, source (rows, cols) uint8, counts [none, own, -1, +1, -2, +2, ...] (2 + 2 radius), own:
    the own stabilize_frame)"""
    npairs = len(depths)
    own = stab.stabilize_frame(images[q], depths[q], Rs[q], ts[q], K, M_own, m_own, mode=mode, q5_mode=q5_mode, iterations=iterations)
    out, mask = own["image"].copy(), own["mask"].copy()
    source = mask.copy()
    counts = [0] * (2 + 2 * radius)
    counts[1] = int(mask.sum())
    for n in neighbour_order(q, npairs, radius):
        sid = source_id(n - q)
        M, m = neighbour_pose(A, c, As, cs, scales, q, n)
        counts[sid] = fill_from(out, mask, source, images[n], depths[n], Rs[n], ts[n], K, M, m, sid, mode, q5_mode, iterations)
    counts[0] = mask.size - sum(counts[1:])  # a skipped offset counts 0
    return dict(image=out, mask=mask, source=source, counts=counts, own=own)
