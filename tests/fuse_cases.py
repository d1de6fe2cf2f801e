"""Inputs of the fusion tests (tests/fuse_spec_numpy.py is the definition): chains of maps and fields built from link_cases.base_case's
recipe, in which pair q + 1's map is roughly a constant times pair q's prediction, so that candidates really agree; the special chain the
GPU test holds the kernels to bit for bit; and the figures of the accuracy scene (link_cases.accuracy_scene) measured on the CPU."""
import numpy as np

import link_cases
import link_spec_numpy as link_spec

SHAPES = link_cases.SHAPES  # (2, 2) ... (150, 200): the edges of the 64 x 16 LDS tile and of a wave
HOLES = [0.0, 0.3, 0.97]
SPECIAL_SHAPES = [(17, 70), (65, 129), (150, 200)]
RATIOS = (1.7, 0.6, 1.3, 0.85, 2.0)  # the units of consecutive pairs; cycled along a chain
BROKEN = {"invalid": dict(ratio=1.3, valid=False), "nan": dict(ratio=float("nan"), valid=True), "negative": dict(ratio=-1.3, valid=True)}


def record(ratio, valid=True):
    """a link record as the fusion reads it (n and agree are not read)"""
    return dict(n=100, ratio=float(ratio), agree=90, valid=bool(valid))


def chain_case(rows, cols, n=3, holes=0.3, salt=0):
    """n pairs.  Fields and the first map are base_case's; map q + 1 is RATIOS[q] times pair q's prediction scattered at the landing pixels
    (over RATIOS[q] times map q where nothing lands), with 3 % noise and 2 % of the pixels half as far again, so that most candidates agree
    and some do not.  Then every map loses its share of holes (exact zeros, as the solve leaves them).
    -> dict(fields [n], maps [n], vs, ws, ks, records [n - 1], K, gamma)"""
    r = np.random.default_rng(7919 * rows + 104729 * cols + 31 * n + salt)
    fields, maps, vs, ws, ks, recs = [], [], [], [], [], []
    base = link_cases.base_case(rows, cols, 0.0, salt=100 + salt)
    K, gamma = base["K"], base["gamma"]
    Z = base["Zp"]
    for q in range(n):
        d = link_cases.base_case(rows, cols, 0.0, salt=200 + salt + q)
        v, w, k = d["v"] * (1.0 + 0.1 * (q % 3)), d["w"] * (1.0 - 0.2 * (q % 2)), (0.0, 0.2, -0.1)[q % 3]
        fields.append(d["F"]), maps.append(Z), vs.append(v), ws.append(w), ks.append(k)
        if q == n - 1:
            break
        c = RATIOS[q % len(RATIOS)]
        z_pred, r2, c2, inside = link_spec.predict(d["F"], Z, v, w, k, K, gamma)
        Zn = c * Z
        Zn[r2[inside], c2[inside]] = c * z_pred[inside]
        Zn = Zn * np.exp(r.normal(0.0, 0.03, (rows, cols)))
        Zn[r.uniform(size=(rows, cols)) < 0.02] *= 1.5
        recs.append(record(c))
        Z = Zn
    for q in range(n):
        maps[q] = maps[q].copy()
        maps[q][r.uniform(size=(rows, cols)) < holes] = 0.0
    return dict(fields=fields, maps=maps, vs=vs, ws=ws, ks=ks, records=recs, K=K, gamma=gamma)


def collision_field(rows, cols):
    """fu alternates 0.4 (even columns) and -0.6 (odd columns), fv = 0: columns 2 m and 2 m + 1 both land on column 2 m"""
    F = np.zeros((rows, cols, 2))
    F[:, 0::2, 0], F[:, 1::2, 0] = 0.4, -0.6
    return F


def special_chain(rows, cols, broken="invalid"):
    """six pairs (rows, cols >= 16):
      pair 0  link_cases.special_case: NaN / inf vectors, vectors leaving every border, landing exactly on the last row and column and half
              a pixel short of leaving
      pair 1  (0, 0) vectors at holes and at own pixels, a NaN vector; a strong v2 < 0: negative z_pred in its splat
      pair 2  a map without a valid pixel
      pair 3  in front of a BROKEN link (`broken`: invalid / nan / negative)
      pair 4  behind it: the collision field; a strong v2 > 0: negative zc in its gather; its link to pair 5 is a power of two
      pair 5  the last pair: no field
    and NaN, +-inf and a negative depth in every map."""
    d, _ = link_cases.special_case(rows, cols)
    ch = chain_case(rows, cols, n=6, holes=0.3, salt=53)
    fields, maps, vs, ws, ks = ch["fields"], ch["maps"], ch["vs"], ch["ws"], ch["ks"]
    fields[0], maps[0], maps[1] = d["F"], d["Zp"], d["Zn"]
    vs[0], ws[0], ks[0] = d["v"], d["w"], d["k"]
    F1 = fields[1]
    holes1 = np.argwhere(~link_spec.valid_depth(maps[1]))[:6]
    own1 = np.argwhere(link_spec.valid_depth(maps[1]))[:6]
    for i, j in list(holes1) + list(own1):
        F1[i, j] = (0.0, 0.0)
    F1[own1[0][0], own1[0][1]] = (-0.0, 0.0)
    F1[12, 12] = (np.nan, 1.0)
    F1[12, 13] = (1.0, -np.inf)
    vs[1] = np.array([0.0, 0.0, -1.45])
    maps[2] = link_cases.empty_case(rows, cols)["Zp"]
    fields[4] = collision_field(rows, cols)
    vs[4] = np.array([0.0, 0.0, 0.9])
    fields[5] = None
    for q in range(6):
        for a, (i, j) in enumerate([(1, 1), (2, 3), (3, 5), (4, 7)]):
            maps[q][i + q, j] = (np.nan, np.inf, -np.inf, -1.5)[a]
    recs = [record(1.7), record(0.6), record(1.3), dict(record(1.0), **BROKEN[broken]), record(2.0)]
    return dict(fields=fields, maps=maps, vs=vs, ws=ws, ks=ks, records=recs, K=ch["K"], gamma=ch["gamma"])


# ---- the accuracy scene (link_cases.accuracy_scene: oracle solve, spec link, spec fusion) -----------------------------------------------------------------
# measured on the CPU (tests/test_fuse_cpu.py: test_fill_accuracy_through_the_oracle prints them): (a) the largest 95th-percentile relative
# error of the PREV-filled pixels over the pairs, (b) the smallest share of a pair's holes that get a value; and the bounds the CPU and the GPU
# tests hold them to -- (a) plus half of it, (b) less 5 points -- for the last-digit differences of the GPU solve
ACC_PREV_P95_MEASURED = 0.131457
ACC_FILLED_MEASURED = 0.730083
ACC_PREV_P95_BOUND = 1.5 * ACC_PREV_P95_MEASURED
ACC_FILLED_BOUND = ACC_FILLED_MEASURED - 0.05


def fill_statistics(fused_out, maps, truth):
    """per pair: dict(holes, unit -- the median of own / truth --, filled: the share of holes with a value, share_prev, share_next, and own /
    prev / next: (median, 95th percentile) of the relative error against unit * truth at the own pixels, the PREV-filled and the NEXT-filled ones)"""
    out = []
    for p, Z in enumerate(maps):
        own = link_spec.valid_depth(Z)
        unit = np.median(Z[own] / truth[own])
        fl, f = fused_out["flags"][p], fused_out["fused"][p]
        err = np.abs(f / (unit * truth) - 1.0)
        by_prev, by_next = ~own & ((fl & 2) != 0), ~own & ((fl & 2) == 0) & ((fl & 4) != 0)
        pct = lambda m: (float(np.median(err[m])), float(np.percentile(err[m], 95))) if m.any() else (float("nan"), float("nan"))
        holes = int((~own).sum())
        out.append(dict(holes=holes, unit=float(unit), filled=float((by_prev | by_next).sum()) / max(holes, 1), share_prev=float(by_prev.sum()) / max(holes, 1),
                        share_next=float(by_next.sum()) / max(holes, 1), own=pct(own), prev=pct(by_prev), next=pct(by_next)))
    return out
