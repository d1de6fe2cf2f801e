"""CPU: the fusion of a clip's depth maps as tests/fuse_spec_numpy.py defines it -- own depths kept, exact cases, the z-buffer's order
independence, the link's agree count seen from the fusion, broken links, the golden fixture, the accuracy of the filled depths through the
oracle's solve -- and its ABI (include/rsdsfm_fuse.h): exported by both library builds, the kernels without a private segment."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fuse_cases as cases
import fuse_spec_numpy as spec
import link_cases
import link_spec_numpy as link_spec
from conftest import ROOT

NEW_SYMBOLS = {"rsdsfm_fuse_params_init", "rsdsfm_fuse_depths_dev"}
GOLDEN = os.path.join(ROOT, "tests", "golden", "golden_fuse_v1.npz")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _fuse(ch, **kw):
    return spec.fuse(ch["fields"], ch["maps"], ch["vs"], ch["ws"], ch["ks"], ch["records"], ch["K"], ch["gamma"], **kw)


# ---- properties of the definition -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_own_depths_are_kept_and_the_record_adds_up(shape):
    rows, cols = shape
    for holes in cases.HOLES:
        ch = cases.chain_case(rows, cols, 3, holes)
        out = _fuse(ch)
        for p in range(3):
            own = link_spec.valid_depth(ch["maps"][p])
            fl, f, rec = out["flags"][p], out["fused"][p], out["records"][p]
            assert np.array_equal(_bits(f)[own], _bits(ch["maps"][p])[own]) and np.array_equal((fl & spec.OWN) != 0, own)
            assert rec["own"] + rec["filled_prev"] + rec["filled_next"] + rec["left"] == rows * cols and rec["own"] == int(own.sum())
            assert np.array_equal(link_spec.valid_depth(f), (fl & 7) != 0) and np.array_equal(_bits(f)[(fl & 7) == 0], np.zeros(rec["left"], dtype=np.uint64))
            # a candidate agrees only where it exists, and the one that is the fused value agrees
            assert not np.any(((fl & spec.PREV_AGREES) != 0) & ((fl & spec.PREV) == 0)) and not np.any(((fl & spec.NEXT_AGREES) != 0) & ((fl & spec.NEXT) == 0))
            by_prev, by_next = ~own & ((fl & spec.PREV) != 0), ~own & ((fl & spec.PREV) == 0) & ((fl & spec.NEXT) != 0)
            assert np.all(fl[by_prev] & spec.PREV_AGREES) and np.all(fl[by_next] & spec.NEXT_AGREES)
            if p == 0:
                assert not np.any(fl & spec.PREV) and np.all(out["splat"][0][~((out["flags"][1] & spec.PREV) != 0)] == spec.NOTHING)
            if p == 2:
                assert not np.any(fl & spec.NEXT)


def test_chains_fill_most_holes_and_candidates_mostly_agree():
    """the chain cases are what they claim: at 30 % holes most holes get a value from either side, most own pixels are confirmed, some
    are contradicted (the planted pixels half as far again)"""
    ch = cases.chain_case(150, 200, 3, 0.3)
    out = _fuse(ch)
    mid = out["records"][1]
    holes = 150 * 200 - mid["own"]
    assert mid["filled_prev"] > 0.5 * holes and mid["filled_next"] > 0 and mid["left"] < 0.2 * holes
    assert mid["confirmed"] > 0.8 * mid["own"] and 0 < mid["contradicted"] < 0.2 * mid["own"]
    assert out["records"][0]["filled_prev"] == 0 and out["records"][2]["filled_next"] == 0 and out["records"][0]["filled_next"] > 0


def test_full_maps_are_returned_as_they_are():
    ch = cases.chain_case(65, 129, 4, 0.0)
    out = _fuse(ch)
    for p in range(4):
        assert np.array_equal(_bits(out["fused"][p]), _bits(ch["maps"][p]))
        r = out["records"][p]
        assert r["own"] == 65 * 129 and r["filled_prev"] == r["filled_next"] == r["left"] == 0


def test_pure_shift_and_power_of_two_ratio_move_the_neighbours_values_exactly():
    """w0 = w1 = v2 = 0 and the vector (1, 0): z_pred = z exactly and the landing pixel is one column to the right, so with ratio 2^-2 the
    PREV candidate at (i, j) is 0.25 * Z_0[i, j - 1] and the NEXT candidate of pair 0 at (i, j) is Z_1[i, j + 1] / 0.25, bit for bit"""
    rows, cols = 9, 21
    r = np.random.default_rng(3)
    Z0, Z1 = r.uniform(0.5, 2.0, (rows, cols)), r.uniform(0.5, 2.0, (rows, cols))
    F = np.zeros((rows, cols, 2))
    F[..., 0] = 1.0
    v, w = np.array([0.02, 0.01, 0.0]), np.array([0.0, 0.0, 0.03])
    hole0, hole1 = np.zeros((rows, cols), dtype=bool), np.zeros((rows, cols), dtype=bool)
    hole0[2:5, 3:9], hole1[4:8, 6:15] = True, True
    A, B = np.where(hole0, 0.0, Z0), np.where(hole1, 0.0, Z1)
    out = spec.fuse([F], [A, B], [v, v], [w, w], [0.3, 0.3], [cases.record(0.25)], link_cases.camera(rows, cols), 0.8)
    want1 = B.copy()
    src = np.zeros_like(A)
    src[:, 1:] = A[:, :-1]
    take = hole1 & (src > 0)
    want1[take] = 0.25 * src[take]
    assert np.array_equal(_bits(out["fused"][1]), _bits(want1)) and out["records"][1]["filled_prev"] == int(take.sum()) > 0
    assert out["records"][1]["left"] == int((hole1 & ~take).sum())
    want0 = A.copy()
    nxt = np.zeros_like(B)
    nxt[:, :-1] = B[:, 1:]
    take0 = hole0 & (nxt > 0)
    want0[take0] = nxt[take0] / 0.25
    assert np.array_equal(_bits(out["fused"][0]), _bits(want0)) and out["records"][0]["filled_next"] == int(take0.sum()) > 0
    plane = np.full((rows, cols), spec.NOTHING, dtype=np.uint64)
    plane[:, 1:] = np.where(A[:, :-1] > 0, _bits(0.25 * A[:, :-1]), spec.NOTHING)
    assert np.array_equal(out["splat"][0], plane)


def test_collisions_keep_the_smaller_offer_in_any_order():
    rows, cols = 12, 30
    r = np.random.default_rng(5)
    Z = r.uniform(0.5, 2.0, (rows, cols))
    F = cases.collision_field(rows, cols)
    v, w = np.array([0.02, 0.01, 0.0]), np.array([0.0, 0.0, 0.03])
    K = link_cases.camera(rows, cols)
    where, zf = spec.splat_offers(F, Z, v, w, 0.0, 1.0, K, 0.8)
    assert where.size == rows * cols and np.array_equal(np.bincount(where, minlength=rows * cols).reshape(rows, cols)[:, 0::2], np.full((rows, cols // 2), 2))
    plane = spec.apply_offers((rows, cols), where, zf)
    assert np.array_equal(plane[:, 0::2].view(np.float64), np.minimum(Z[:, 0::2], Z[:, 1::2])) and np.all(plane[:, 1::2] == spec.NOTHING)
    for seed in range(5):
        perm = np.random.default_rng(seed).permutation(where.size)
        assert np.array_equal(spec.apply_offers((rows, cols), where[perm], zf[perm]), plane)
    assert np.array_equal(spec.splat_plane(F, Z, v, w, 0.0, 1.0, K, 0.8), plane)


@pytest.mark.parametrize("broken", sorted(cases.BROKEN))
def test_a_broken_link_passes_nothing_on_either_side(broken):
    ch = cases.chain_case(33, 70, 3, 0.3)
    ch["records"][0] = dict(cases.record(1.0), **cases.BROKEN[broken])
    out = _fuse(ch)
    assert np.all(out["splat"][0] == spec.NOTHING)
    assert not np.any(out["flags"][0] & (spec.NEXT | spec.NEXT_AGREES)) and not np.any(out["flags"][1] & (spec.PREV | spec.PREV_AGREES))
    assert out["records"][0]["filled_next"] == 0 and out["records"][1]["filled_prev"] == 0
    assert out["records"][1]["filled_next"] > 0 and out["records"][2]["filled_prev"] > 0  # the other link still works
    assert np.array_equal(_bits(out["fused"][0]), _bits(np.where(link_spec.valid_depth(ch["maps"][0]), ch["maps"][0], 0.0)))


def test_one_pair_is_its_own_map():
    ch = cases.chain_case(17, 70, 1, 0.3)
    out = spec.fuse([], ch["maps"], ch["vs"], ch["ws"], ch["ks"], [], ch["K"], ch["gamma"])
    assert np.array_equal(_bits(out["fused"][0]), _bits(ch["maps"][0])) and out["splat"] == [] and not np.any(out["flags"][0] & ~np.uint8(spec.OWN))


@pytest.mark.parametrize("shape", cases.SPECIAL_SHAPES)
def test_special_chain_exercises_what_it_claims(shape):
    rows, cols = shape
    ch = cases.special_chain(rows, cols)
    out = _fuse(ch)
    maps, fl = ch["maps"], out["flags"]
    for q in range(6):
        bad = maps[q][[1 + q, 2 + q, 3 + q, 4 + q], [1, 3, 5, 7]]
        assert np.isnan(bad[0]) or q == 2
        assert not np.any(fl[q][[1 + q, 2 + q, 3 + q, 4 + q], [1, 3, 5, 7]] & spec.OWN)
    assert not link_spec.valid_depth(maps[2]).any() and out["records"][2]["own"] == 0 and out["records"][2]["filled_prev"] > 0  # every value of pair 2 is a neighbour's
    z_pred1 = link_spec.predict(ch["fields"][1], maps[1], ch["vs"][1], ch["ws"][1], ch["ks"][1], ch["K"], ch["gamma"])[0]
    assert (z_pred1[link_spec.valid_depth(maps[1])] < 0).mean() > 0.2
    assert (z_pred1[link_spec.valid_depth(maps[1])] > 0).mean() > 0.02
    # pair 4: negative zc at pixels whose landing pixel carries a depth; collisions in its splat
    with np.errstate(all="ignore"):
        qx, qy, b = link_spec.point_terms(ch["fields"][4], ch["K"], ch["gamma"], ch["ks"][4])
        _, r2, c2, inside = link_spec.predict(ch["fields"][4], maps[4], ch["vs"][4], ch["ws"][4], ch["ks"][4], ch["K"], ch["gamma"])
        z2 = maps[5][r2, c2]
        zc = (z2 / ch["records"][4]["ratio"] - b * ch["vs"][4][2]) / (1.0 + b * (ch["ws"][4][0] * qy - ch["ws"][4][1] * qx))
    neg = (zc[inside & link_spec.valid_depth(z2)] < 0).mean()
    assert 0.2 < neg < 0.98, neg
    where, _ = spec.splat_offers(ch["fields"][4], maps[4], ch["vs"][4], ch["ws"][4], ch["ks"][4], 2.0, ch["K"], ch["gamma"])
    assert np.bincount(where).max() == 2
    # the broken link 3: nothing across it
    assert np.all(out["splat"][3] == spec.NOTHING) and not np.any(fl[3] & spec.NEXT) and not np.any(fl[4] & spec.PREV)
    assert out["records"][4]["filled_next"] > 0 and out["records"][5]["filled_prev"] > 0 and out["records"][0]["filled_next"] > 0
    # (0, 0) vectors offer nothing and gather nothing: the splat of pair 1 never lands a (0, 0) pixel's value on itself
    zero = (ch["fields"][1][..., 0] == 0) & (ch["fields"][1][..., 1] == 0)
    assert zero.sum() >= 12 and not np.any(fl[1][zero] & spec.NEXT)
    nanv = ~np.isfinite(ch["fields"][0]).all(-1)
    assert nanv.sum() >= 3 and not np.any(fl[0][nanv] & spec.NEXT)
    for px in [(0, 4), (rows - 1, 4), (5, 0), (5, cols - 1), (10, 10), (11, 10)]:  # link_cases.special_case's vectors that leave the frame
        assert not fl[0][px] & spec.NEXT, px


# ---- the golden fixture ---------------------------------------------------------------------------------------------------------------------------------
def test_golden_fixture_is_the_spec():
    """tests/golden/make_golden_fuse.py wrote the (17, 70) special chain and a (3, 5) chain with what the spec makes of them; recomputed
    here, so an edit of the spec or of the cases cannot pass unnoticed"""
    assert os.path.getsize(GOLDEN) < 200 * 1024
    g = np.load(GOLDEN)
    for tag, ch, kw in (("special", cases.special_chain(17, 70), {}), ("small", cases.chain_case(3, 5, 3, 0.3), dict(tol=0.01))):
        out = _fuse(ch, **kw)
        n = len(ch["maps"])
        assert np.array_equal(_bits(np.stack(ch["maps"])), g[tag + "_maps"]), tag
        assert np.array_equal(_bits(np.stack(out["fused"])), g[tag + "_fused"]) and np.array_equal(np.stack(out["flags"]), g[tag + "_flags"]), tag
        assert np.array_equal(np.stack(out["splat"]), g[tag + "_splat"]), tag
        assert np.array_equal(np.array([[r[k] for k in spec.RECORD_FIELDS] for r in out["records"]], dtype=np.int64), g[tag + "_records"]) and n == len(g[tag + "_records"])
    assert g["special_records"][:, 1].sum() > 0 and g["special_records"][:, 2].sum() > 0 and g["special_records"][:, 4].sum() > 0


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_fuse_symbols_are_exported(rsdsfm, arith):
    lib = rsdsfm.load_library(arith=arith)
    names = rsdsfm.fuse_declared_symbols()
    assert set(names) == NEW_SYMBOLS
    assert not [n for n in names if not hasattr(lib, n)]
    for other in (rsdsfm.declared_symbols(), rsdsfm.video_declared_symbols(), rsdsfm.rectify_video_declared_symbols(), rsdsfm.flow_declared_symbols(),
                  rsdsfm.rectify_dense_declared_symbols(), rsdsfm.flow_check_declared_symbols(), rsdsfm.trajectory_declared_symbols()):
        assert not NEW_SYMBOLS & set(other)
    assert rsdsfm.fuse_default_params() == dict(tol=link_spec.TOL_DEFAULT)
    assert ctypes.sizeof(rsdsfm.FuseParams) == 16 and ctypes.sizeof(rsdsfm.FuseRecord) == 48
    assert os.path.exists(rsdsfm.FUSE_HEADER_PATH)
    assert [k for k, _ in rsdsfm.FuseRecord._fields_] == list(spec.RECORD_FIELDS)
    assert (rsdsfm.FUSE_OWN, rsdsfm.FUSE_PREV, rsdsfm.FUSE_NEXT, rsdsfm.FUSE_PREV_AGREES, rsdsfm.FUSE_NEXT_AGREES) == (spec.OWN, spec.PREV, spec.NEXT, spec.PREV_AGREES,
                                                                                                                        spec.NEXT_AGREES)


def test_fuse_kernels_have_no_private_segment(tmp_path):
    """hipcc -S of fuse_kernels.hip, its metadata: both kernels with a zero private segment, no VGPR and no SGPR spills"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rs-aware-differential-sfm_amd", "csrc", "fuse_kernels.hip")
    out = tmp_path / "fuse_kernels.s"
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), src,
                        "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    txt = out.read_text()
    meta = re.search(r"amdhsa.kernels:(.*?)\n\.\.\.", txt, flags=re.S).group(1)
    for kernel in ("fuse_splat_kernel", "fuse_merge_kernel"):
        assert kernel in meta, kernel
    for key in (".private_segment_fixed_size", ".sgpr_spill_count", ".vgpr_spill_count"):
        vals = [int(x) for x in re.findall(re.escape(key) + r":\s+(\d+)", meta)]
        assert len(vals) == 2 and not any(vals), (key, vals)


def test_evaluate_refuses_fusion_without_the_trajectory(rsdsfm):
    """fuse=True needs the links: ValueError before anything touches a GPU (the solver is never used)"""
    frames = np.zeros((3, 8, 8), dtype=np.uint8)
    with pytest.raises(ValueError, match="trajectory"):
        rsdsfm.evaluate.evaluate_real_sequence(None, frames, camera=(8.0, 8.0, 4.0, 4.0), fuse=True, trajectory=False)


# ---- accuracy -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def accuracy_solution(rsdsfm, oracle):
    """link_cases' accuracy scene solved by the oracle (as tests/test_link_cpu.py does), linked by the link's spec: computed once"""
    O = oracle
    sc = link_cases.accuracy_scene(rsdsfm.synth)
    rows, cols, K, gamma = link_cases.ACC_ROWS, link_cases.ACC_COLS, sc["K"], sc["gamma"]
    sol = []
    for f in sc["fields"]:
        qf, uf, qpx, fpx = O.flatten(f, *K, gamma)
        af, akf = O.get_alpha(fpx, rows, gamma), O.get_alpha_k(qpx, fpx, rows, gamma)
        ro = O.ransac(qf, uf, af, akf, False, link_cases.ACC_TRIALS, link_cases.ACC_TOL, O.sample_indices(len(qf), link_cases.ACC_TRIALS, link_cases.ACC_SOLVE_SEED),
                      depth_mode=1)
        refo = O.refine(uf, ro["inliers"], ro["alpha"], ro["alpha_k"], ro["v"], ro["w"], ro["k"], False, 1, ro["inlier_idx"])
        inl, v, _ = O.canonicalize_sign(refo["inliers"], refo["v"])
        dm, _, _ = O.scatter_depth(inl, *K, rows, cols)
        sol.append(dict(v=v, w=refo["w"], k=refo["k"], Z=dm))
    links = [link_spec.link(sc["fields"][q], sol[q]["Z"], sol[q]["v"], sol[q]["w"], sol[q]["k"], sol[q + 1]["Z"], K, gamma) for q in range(2)]
    ch = dict(fields=sc["fields"], maps=[s["Z"] for s in sol], vs=[s["v"] for s in sol], ws=[s["w"] for s in sol], ks=[s["k"] for s in sol], records=links, K=K,
              gamma=gamma)
    return ch, _fuse(ch), rsdsfm.synth.scene_depth(rows, cols)


def test_next_agreement_is_the_links_agree_count(accuracy_solution):
    """at the pixels that have an own depth and a NEXT candidate, "the candidate agrees with the own depth" is the link's "the ratio agrees
    with the median" up to the roundings of the two divisions: the counts differ by at most 1 per link"""
    ch, out, _ = accuracy_solution
    for q in range(2):
        fl = out["flags"][q]
        both = ((fl & spec.OWN) != 0) & ((fl & spec.NEXT) != 0)
        agree = int((both & ((fl & spec.NEXT_AGREES) != 0)).sum())
        print("link %d: the link's agree %d of n %d; NEXT_AGREES at OWN and NEXT pixels %d of %d" % (q, ch["records"][q]["agree"], ch["records"][q]["n"], agree, int(both.sum())))
        assert abs(agree - ch["records"][q]["agree"]) <= 1


def test_fill_accuracy_through_the_oracle(accuracy_solution):
    """The accuracy scene of link_cases (96 x 128, three pairs; oracle solve, spec link, spec fusion) against synth.scene_depth in each
    pair's unit (the median of own / truth).  Measured here on the CPU -- see the printed table; the figures are recorded in
    tests/fuse_cases.py (ACC_PREV_P95_MEASURED, ACC_FILLED_MEASURED) and repeated in DESIGN.md section 12, "Depth fusion".  The bounds,
    here and for the GPU solve (tests/test_gpu_fuse.py): the largest 95th-percentile error of PREV-filled pixels plus half of it, and the
    smallest share of holes filled less 5 points.  What justifies OWN > PREV > NEXT: on pair 1 the PREV candidates at holes have a smaller
    95th-percentile error than the NEXT candidates at holes."""
    ch, out, truth = accuracy_solution
    stats = cases.fill_statistics(out, ch["maps"], truth)
    for p, s in enumerate(stats):
        print("pair %d: own %d holes %d filled %.4f (PREV %.4f NEXT %.4f) left %d | rel. error median / p95: own %.4f / %.4f, PREV-filled %.4f / %.4f, NEXT-filled %.4f / %.4f"
              % (p, out["records"][p]["own"], s["holes"], s["filled"], s["share_prev"], s["share_next"], out["records"][p]["left"], s["own"][0], s["own"][1],
                 s["prev"][0], s["prev"][1], s["next"][0], s["next"][1]))
        assert out["records"][p]["filled_prev"] + out["records"][p]["filled_next"] + out["records"][p]["left"] == s["holes"]
    prev_p95 = max(s["prev"][1] for s in stats[1:])
    filled = min(s["filled"] for s in stats)
    print("recorded figures: ACC_PREV_P95_MEASURED = %.6f  ACC_FILLED_MEASURED = %.6f" % (prev_p95, filled))
    # the precedence: ALL candidates at the holes of pair 1, PREV against NEXT
    own1 = link_spec.valid_depth(ch["maps"][1])
    unit = stats[1]["unit"]
    fl = out["flags"][1]
    zprev = np.where(out["splat"][0] != spec.NOTHING, out["splat"][0], np.uint64(0)).view(np.float64)
    znext, nxt = spec.gather_candidate(ch["fields"][1], ch["maps"][1], ch["vs"][1], ch["ws"][1], ch["ks"][1], ch["records"][1]["ratio"], ch["maps"][2], ch["K"], ch["gamma"])
    at_prev, at_next = ~own1 & ((fl & spec.PREV) != 0), ~own1 & nxt
    assert np.array_equal(nxt, (fl & spec.NEXT) != 0)
    e_prev, e_next = np.abs(zprev[at_prev] / (unit * truth[at_prev]) - 1.0), np.abs(znext[at_next] / (unit * truth[at_next]) - 1.0)
    print("pair 1, candidates at holes: PREV %d median %.4f p95 %.4f | NEXT %d median %.4f p95 %.4f"
          % (e_prev.size, np.median(e_prev), np.percentile(e_prev, 95), e_next.size, np.median(e_next), np.percentile(e_next, 95)))
    assert np.percentile(e_prev, 95) < np.percentile(e_next, 95)
    assert abs(prev_p95 - cases.ACC_PREV_P95_MEASURED) <= 0.01 * cases.ACC_PREV_P95_MEASURED  # the recorded numbers are this computation's
    assert abs(filled - cases.ACC_FILLED_MEASURED) <= 0.01 * cases.ACC_FILLED_MEASURED
    assert prev_p95 <= cases.ACC_PREV_P95_BOUND and filled >= cases.ACC_FILLED_BOUND
