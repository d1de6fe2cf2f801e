"""The fusion of a clip's depth maps (include/rsdsfm_fuse.h), defined in float64 numpy: the kernels of csrc/fuse_kernels.hip reproduce every
output bit for bit.  Every operation is rounded once and none is fused (the library is built with -ffp-contract=off).  The per-pixel terms,
the prediction and the validity rule are tests/link_spec_numpy.py's (point_terms, predict, valid_depth), whose numbered steps are cited.

A pair's depth map carries a depth only where the pair's RANSAC kept the pixel.  Its neighbours measured some of the holes: pair p - 1's
depths, moved to that pair's second capture (which is pair p's first) by its solved motion, and pair p + 1's depths, looked up where pair
p's flow lands and moved back.  The link's ratio converts between the pairs' units.

n >= 1 pairs with fields F_p (rows x cols x 2), depth maps Z_p ((rows, cols) here; column-major on the device), final motions (v, w, k)_p,
K = (fx, fy, cx, cy), and the n - 1 link records (link l relates pairs l and l + 1: ratio = unit of pair l + 1 over unit of pair l).
    link l is USABLE iff valid is set and ratio is finite and > 0 (chain's rule)
    a vector is USABLE iff both components are finite and not both are exactly 0 ((0, 0) is what the flow check writes for a rejected pixel)

PREV, the candidate from the previous pair (a splat): for pair p >= 1 with link p - 1 usable, r its ratio.  Every pixel (i, j) of pair p - 1
with Z_{p-1}[i, j] valid and a usable vector: steps 1 - 4 of the link with pair p - 1's motion give z_pred and the landing pixel (r2, c2);
if that is inside and zf = z_pred * r is valid, the pixel OFFERS zf to (r2, c2) of pair p.  Among the offers to one pixel the smallest wins
(the nearest surface).  splat[p - 1] is the (rows, cols) uint64 plane of the winners' bit patterns, all ones where nothing landed (a valid
depth is a positive finite double: its pattern orders as an integer and is below all ones).

NEXT, the candidate from the next pair (a gather): for pair p <= n - 2 with link p usable, r its ratio.  Every pixel (i, j) of pair p with
a usable vector and an inside landing pixel (r2, c2) (step 4), with pair p's motion and the pixel's own (qx, qy, b) (steps 1 - 2):
    z2 = Z_{p+1}[r2, c2],   zc = (z2 / r - b * v2) / (1.0 + b * (w0 * qy - w1 * qx))        (step 3 solved for z)
the candidate is zc and exists iff z2 and zc are valid.  Computed at every pixel, not only at holes.

fused[i, j] = Z_p[i, j] where that is valid (OWN; bit for bit), else the PREV candidate, else the NEXT candidate, else +0.0.
flags[i, j] (uint8): bit 0 OWN, bit 1 PREV exists, bit 2 NEXT exists, bit 3 PREV_AGREES, bit 4 NEXT_AGREES; a candidate a agrees with the
fused value f iff a <= f * (1.0 + tol) and a * (1.0 + tol) >= f (a candidate that IS the fused value satisfies both).
Record per pair: own, filled_prev (not OWN, PREV), filled_next (neither, NEXT), confirmed (OWN and a candidate that agrees), contradicted
(OWN and a candidate that exists and does not agree; a pixel can be both), left (no value).
"""
import numpy as np

from link_spec_numpy import TOL_DEFAULT, point_terms, predict, valid_depth

OWN, PREV, NEXT, PREV_AGREES, NEXT_AGREES = 1, 2, 4, 8, 16
NOTHING = np.uint64(0xFFFFFFFFFFFFFFFF)
RECORD_FIELDS = ("own", "filled_prev", "filled_next", "confirmed", "contradicted", "left")


def usable_link(rec):
    r = np.float64(rec["ratio"])
    return bool(rec["valid"]) and bool(np.isfinite(r)) and bool(r > 0.0)


def usable_vector(F):
    F = np.asarray(F, dtype=np.float64)
    return np.isfinite(F[..., 0]) & np.isfinite(F[..., 1]) & ~((F[..., 0] == 0.0) & (F[..., 1] == 0.0))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def splat_offers(F, Z, v, w, k, ratio, K, gamma, global_shutter=False):
    """the offers of one pair to the next: (flat landing index, zf) of every offering pixel, in pixel order"""
    Z = np.asarray(Z, dtype=np.float64)
    cols = Z.shape[1]
    z_pred, r2, c2, inside = predict(F, Z, v, w, k, K, gamma, global_shutter)
    with np.errstate(all="ignore"):
        zf = z_pred * np.float64(ratio)
        ok = valid_depth(Z) & usable_vector(F) & inside & valid_depth(zf)
    return (r2 * cols + c2)[ok], zf[ok]


def apply_offers(shape, where, zf):
    """the z-buffer: the smallest offer per pixel as a bit pattern, all ones where there is none; independent of the offers' order"""
    plane = np.full(shape[0] * shape[1], NOTHING, dtype=np.uint64)
    np.minimum.at(plane, where, _bits(zf))
    return plane.reshape(shape)


def splat_plane(F, Z, v, w, k, ratio, K, gamma, global_shutter=False):
    where, zf = splat_offers(F, Z, v, w, k, ratio, K, gamma, global_shutter)
    return apply_offers(np.asarray(Z).shape, where, zf)


def gather_candidate(F, Z, v, w, k, ratio, Z_next, K, gamma, global_shutter=False):
    """(zc, exists) per pixel of pair p"""
    Z, Z_next = np.asarray(Z, dtype=np.float64), np.asarray(Z_next, dtype=np.float64)
    v, w = np.asarray(v, dtype=np.float64), np.asarray(w, dtype=np.float64)
    _, r2, c2, inside = predict(F, Z, v, w, k, K, gamma, global_shutter)
    with np.errstate(all="ignore"):
        qx, qy, b = point_terms(F, K, gamma, k, global_shutter)
        z2 = Z_next[r2, c2]
        zc = (z2 / np.float64(ratio) - b * v[2]) / (1.0 + b * (w[0] * qy - w[1] * qx))
        exists = usable_vector(F) & inside & valid_depth(z2) & valid_depth(zc)
    return np.where(exists, zc, 0.0), exists


def fuse(fields, maps, vs, ws, ks, records, K, gamma, global_shutter=False, tol=TOL_DEFAULT):
    """-> dict(fused [n] (rows, cols) float64, flags [n] (rows, cols) uint8, splat [n - 1] (rows, cols) uint64, records [n] dicts).
    fields: n or n - 1 (the last pair's field is not read); records: the n - 1 link records (dicts with ratio and valid)."""
    maps = [np.asarray(z, dtype=np.float64) for z in maps]
    n = len(maps)
    shape = maps[0].shape
    assert n >= 1 and len(records) == n - 1 and len(fields) in (n - 1, n) and all(z.shape == shape for z in maps)
    onetol = np.float64(1.0) + np.float64(tol)
    splat = [splat_plane(fields[l], maps[l], vs[l], ws[l], ks[l], records[l]["ratio"], K, gamma, global_shutter) if usable_link(records[l])
             else np.full(shape, NOTHING, dtype=np.uint64) for l in range(n - 1)]
    fused, flags, recs = [], [], []
    for p in range(n):
        own = valid_depth(maps[p])
        prev = splat[p - 1] != NOTHING if p >= 1 else np.zeros(shape, dtype=bool)
        zprev = np.where(prev, splat[p - 1], np.uint64(0)).view(np.float64) if p >= 1 else np.zeros(shape)
        if p <= n - 2 and usable_link(records[p]):
            znext, nxt = gather_candidate(fields[p], maps[p], vs[p], ws[p], ks[p], records[p]["ratio"], maps[p + 1], K, gamma, global_shutter)
        else:
            znext, nxt = np.zeros(shape), np.zeros(shape, dtype=bool)
        f = np.where(own, maps[p], np.where(prev, zprev, np.where(nxt, znext, 0.0)))
        with np.errstate(all="ignore"):
            pa = prev & (zprev <= f * onetol) & (zprev * onetol >= f)
            na = nxt & (znext <= f * onetol) & (znext * onetol >= f)
        fl = (own * OWN + prev * PREV + nxt * NEXT + pa * PREV_AGREES + na * NEXT_AGREES).astype(np.uint8)
        fused.append(f)
        flags.append(fl)
        recs.append(dict(own=int(own.sum()), filled_prev=int((~own & prev).sum()), filled_next=int((~own & ~prev & nxt).sum()),
                         confirmed=int((own & (pa | na)).sum()), contradicted=int((own & ((prev & ~pa) | (nxt & ~na))).sum()),
                         left=int((~own & ~prev & ~nxt).sum())))
    return dict(fused=fused, flags=flags, splat=splat, records=recs)
