"""GPU: the colour-consistent plate (include/rsdsfm_plate_medoid.h) bit for bit against its definition (tests/plate_medoid_spec_numpy.py) in both
library builds -- the medoid call at the shapes where the 16 x 64 tile can go wrong and at every layer count where another instance of its kernel
runs, the constructed cases with hand answers (the impulse's 3 x 3 footprint across tile borders among them), a seeded random campaign, the gray
call against rsdsfm_plate_median_dev, shuffled layers, the context's knob through the frame, clip and erase calls against the golden fixture, the
public calls made one after another and tests/erase_spec_numpy.py, and argument errors.  The guarded, never preset planes are
tests/test_gpu_plate.py's: 16 guard bytes behind every plane, the inputs verified unchanged."""
import functools
import os

import numpy as np
import pytest

import denoise_cases as dcases
import erase_spec_numpy as erase
import plate_cases as cases
import plate_medoid_cases as mcases
import plate_medoid_spec_numpy as spec
from test_gpu_plate import GOLDEN as MEDIAN_GOLDEN
from test_gpu_plate import GUARD, _clip, _collect, _frame, _frame_kw, _golden, _guarded, _outputs, _same, _video

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_plate_medoid_v1.npz")


def _estimate(torch, call, ref, rmask, layers, records=None, with_votes=True, with_moving=True, with_counts=True, **kw):
    """one rsdsfm_plate_medoid_dev (call = s.plate_medoid_dev; or s.plate_median_dev) on guarded planes, the outputs never preset -> the collected
    outputs"""
    dev = torch.device("cuda", 0)
    rows, cols = rmask.shape
    ch = 1 if ref.ndim == 2 else 3
    (d_ref, g_ref), (d_rm, g_rm) = _guarded(torch, dev, ref), _guarded(torch, dev, rmask)
    d_l = [(_guarded(torch, dev, i), _guarded(torch, dev, m)) for i, m in layers]
    d_rec = None
    if records is not None and len(layers):
        d_rec = torch.full((8 * len(layers) + 2,), -1, dtype=torch.int64, device=dev)
        d_rec[1:-1] = torch.from_numpy(np.ascontiguousarray(records, dtype=np.uint64).reshape(-1).view(np.int64)).to(dev)
    planes, cnt = _outputs(torch, dev, ref.shape, (rows, cols))
    torch.cuda.synchronize()
    call(d_ref.data_ptr(), d_rm.data_ptr(), [i.data_ptr() for (i, _), _ in d_l], [m.data_ptr() for _, (m, _) in d_l], ch, rows, cols, planes[0][0].data_ptr(),
         planes[1][0].data_ptr(), planes[2][0].data_ptr() if with_votes else None, planes[3][0].data_ptr() if with_moving else None, cnt[1:].data_ptr() if with_counts else None,
         d_rec[1:].data_ptr() if d_rec is not None else None, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(d_ref.cpu().numpy(), ref) and np.array_equal(d_rm.cpu().numpy(), rmask)  # the inputs are only read
    for ((d_i, _), (d_m, _)), (i, m) in zip(d_l, layers):
        assert np.array_equal(d_i.cpu().numpy(), i) and np.array_equal(d_m.cpu().numpy(), m)
    if d_rec is not None:
        assert np.array_equal(d_rec[1:-1].cpu().numpy().view(np.uint64), np.asarray(records, dtype=np.uint64).reshape(-1)) and d_rec[0] == -1 and d_rec[-1] == -1
    guards = [g_ref, g_rm] + [g for (_, gi), (_, gm) in d_l for g in (gi, gm)]
    return _collect(planes, cnt, guards, with_votes, with_moving, with_counts)


def _run_case(torch, call, case, **kw):
    return _estimate(torch, call, case["ref"], case["rmask"], case["layers"], case["records"], min_overlap=case["min_overlap"], gain_mode=case["gain_mode"],
                     threshold=case["threshold"], min_votes=case["min_votes"], **kw)


# the definition once per input, shared by both builds and never changed
@functools.lru_cache(maxsize=None)
def _wanted(shape, channels, L):
    ref, rmask, ls = cases.median_inputs(shape, channels, L)
    recs = cases.layer_records(channels, L, phase=shape[1])
    threshold, min_votes = cases.median_parameters(shape, L)
    return spec.medoid(ref, rmask, ls, list(recs), threshold=threshold, min_votes=min_votes)


@functools.lru_cache(maxsize=None)
def _wanted_plain(shape, channels):
    ref, rmask, ls = cases.median_inputs(shape, channels, 2, seed=1)
    recs = cases.layer_records(channels, 2, phase=2)  # both clamps: without the gain they must not show
    return spec.medoid(ref, rmask, ls, None), spec.medoid(ref, rmask, ls, list(recs), gain_mode=1, min_overlap=7)


@functools.lru_cache(maxsize=None)
def _wanted_constructed(channels):
    return [(case, mcases.spec_of(case)) for case in mcases.constructed(channels)]


_FRAMES = {}


def _wanted_frame(case, q=None):
    key = (case["name"], q)
    if key not in _FRAMES:
        _FRAMES[key] = spec.run_spec(case, q)
    return _FRAMES[key]


# ---------------------------------------------------------------------------------------------------
# the medoid call
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_call_equals_the_definition(rsdsfm, arith, channels):
    """every shape -- one word, odd sizes, one under, exactly one and one over the tile in both directions, rows that start on every byte of a
    dword, 25 workgroups --; 0, 1, 2, 3, 4, 5, 7, 8, 13 and 14 layers (either side of every instance of the kernel); the five records in turn, the
    gain off, no record; with and without the votes, the flag plane and the counters"""
    import torch

    assert cases.ACC_SHAPES == [(2, 2), (3, 7), (5, 5), (15, 63), (16, 64), (17, 65), (16, 131), (37, 67), (33, 129), (70, 300)]
    assert cases.LAYER_COUNTS == [0, 1, 2, 3, 4, 5, 7, 8, 13, 14]
    seen = np.zeros(4, dtype=np.int64)
    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in cases.ACC_SHAPES:
            for L in cases.LAYER_COUNTS:
                ref, rmask, ls = cases.median_inputs(shape, channels, L)
                threshold, min_votes = cases.median_parameters(shape, L)
                want = _wanted(shape, channels, L)
                got = _estimate(torch, s.plate_medoid_dev, ref, rmask, ls, cases.layer_records(channels, L, phase=shape[1]), threshold=threshold, min_votes=min_votes)
                _same(got, want, (shape, L))
                seen += np.array(want["counts"])
            ref, rmask, ls = cases.median_inputs(shape, channels, 2, seed=1)
            no_record, gain_off = _wanted_plain(shape, channels)
            _same(_estimate(torch, s.plate_medoid_dev, ref, rmask, ls, None), no_record, (shape, "no record"))
            recs = cases.layer_records(channels, 2, phase=2)
            _same(_estimate(torch, s.plate_medoid_dev, ref, rmask, ls, recs, gain_mode=1, min_overlap=7), gain_off, (shape, "gain off"))
            for votes, moving, counts in ((False, True, True), (True, False, True), (True, True, False), (False, False, False), (True, False, False)):
                _same(_estimate(torch, s.plate_medoid_dev, ref, rmask, ls, recs, votes, moving, counts, gain_mode=1, min_overlap=7), gain_off, shape, votes, moving, counts)
        assert rsdsfm.plate_medoid_launches() == 1
    assert (seen > 0).all()


@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_constructed_cases_have_their_known_answers(rsdsfm, arith, channels):
    """tests/plate_medoid_cases.constructed on the kernel: the triple without a majority, all candidates equal, one outlier among fourteen at
    layers 0, 6 and 13, the own frame as the outlier, two candidates, an empty own mask, min_votes 1 and 15, and plate_cases' impulses at every
    corner and edge midpoint of every tile and of the frame (the halo).  Every plane is the definition's, and the hand answers hold"""
    import torch

    with rsdsfm.Solver(0, arith=arith) as s:
        for case, want in _wanted_constructed(channels):
            got = _run_case(torch, s.plate_medoid_dev, case)
            _same(got, want, case["name"])
            for k, hand in case["want"].items():
                assert np.array_equal(np.asarray(got[k]), np.asarray(hand)), (case["name"], k)


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_a_seeded_random_campaign(rsdsfm, arith):
    """200 small cases: shapes up to 40 x 140, gray and BGR, 0 .. 14 layers, sparse to dense masks, records or none, every parameter"""
    import torch

    rng = np.random.default_rng(20240)
    layer_counts, channels = set(), set()
    with rsdsfm.Solver(0, arith=arith) as s:
        for k in range(200):
            case = cases.random_case(rng)
            _same(_run_case(torch, s.plate_medoid_dev, case), mcases.spec_of(case), (k, case["ref"].shape, len(case["layers"])))
            layer_counts.add(len(case["layers"]))
            channels.add(case["ref"].ndim)
    assert layer_counts == set(range(15)) and channels == {2, 3}


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_gray_call_is_the_median_call(rsdsfm, arith):
    """with one channel rsdsfm_plate_medoid_dev is byte for byte rsdsfm_plate_median_dev on the same inputs; with three it is not"""
    import torch

    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in ((3, 7), (17, 65), (37, 67)):
            for L in cases.LAYER_COUNTS:
                ref, rmask, ls = cases.median_inputs(shape, 1, L)
                kw = dict(threshold=cases.median_parameters(shape, L)[0], min_votes=cases.median_parameters(shape, L)[1])
                recs = cases.layer_records(1, L, phase=shape[1])
                _same(_estimate(torch, s.plate_medoid_dev, ref, rmask, ls, recs, **kw), _estimate(torch, s.plate_median_dev, ref, rmask, ls, recs, **kw), (shape, L))
        ref, rmask, ls = cases.median_inputs((37, 67), 3, 4)
        assert not np.array_equal(_estimate(torch, s.plate_medoid_dev, ref, rmask, ls)["image"], _estimate(torch, s.plate_median_dev, ref, rmask, ls)["image"])


@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_order_of_the_layers_does_not_matter(rsdsfm, arith, channels):
    import torch

    rng = np.random.default_rng(5)
    with rsdsfm.Solver(0, arith=arith) as s:
        for L in (5, 14):
            ref, rmask, ls = cases.median_inputs((37, 67), channels, L)
            recs = cases.layer_records(channels, L)
            want = spec.medoid(ref, rmask, ls, list(recs), threshold=30)
            for _ in range(4):
                perm = rng.permutation(L)
                _same(_estimate(torch, s.plate_medoid_dev, ref, rmask, [ls[i] for i in perm], recs[perm], threshold=30), want, perm.tolist())


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_host_convenience_of_the_medoid(rsdsfm, arith):
    ref, rmask, ls = cases.median_inputs((37, 67), 3, 3)
    recs = cases.layer_records(3, 3)
    with rsdsfm.Solver(0, arith=arith) as s:
        img, mask, votes, moving, counts = s.plate_medoid(ref, rmask, ls, recs, threshold=30)
        _same(dict(image=img, mask=mask, votes=votes, moving=moving, counts=counts.tolist()), spec.medoid(ref, rmask, ls, list(recs), threshold=30))
        img, mask, votes, moving, counts = s.plate_medoid(ref, rmask, [])
        _same(dict(image=img, mask=mask, votes=votes, moving=moving, counts=counts.tolist()), spec.medoid(ref, rmask, []))


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_medoid_argument_errors(rsdsfm, arith):
    """the median call's list: every refusal returns RSDSFM_ERR_INVALID and enqueues nothing -- the outputs keep their guard value; after a
    refused call the same call without the fault goes through"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    u8 = lambda value, *shape: torch.full(shape, value, dtype=torch.uint8, device=dev)
    ref, rmask = u8(9, rows, cols, 3), u8(1, rows, cols)
    lay = [u8(9 + j, rows, cols, 3) for j in range(15)]
    lmask = [u8(1, rows, cols) for _ in range(15)]
    out, omask, votes, moving = u8(GUARD, rows, cols + 4, 3), u8(GUARD, rows, cols + 4), u8(GUARD, rows, cols + 4), u8(GUARD, rows, cols + 4)
    counts = torch.full((6,), -1, dtype=torch.int64, device=dev)
    rec = torch.zeros(8 * 15 + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    p = lambda ts: [t.data_ptr() for t in ts]
    with rsdsfm.Solver(0, arith=arith) as s:
        def med(R=ref.data_ptr(), mR=rmask.data_ptr(), L=p(lay[:2]), mL=p(lmask[:2]), n=None, ch=3, r=rows, c=cols, rc=rec.data_ptr(), mo=0, gm=0, th=24, mv=3,
                o=out.data_ptr(), k=omask.data_ptr(), v=votes.data_ptr(), f=moving.data_ptr(), cnt=counts[1:].data_ptr()):
            return s.plate_medoid_dev(R, mR, L, mL, ch, r, c, o, k, v, f, cnt, rc, mo, gm, th, mv, nlayers=n)

        bads = (dict(R=0), dict(mR=0), dict(o=0), dict(k=0), dict(L=None, n=2), dict(mL=None, n=2), dict(L=[lay[0].data_ptr(), 0]), dict(mL=[0, lmask[1].data_ptr()]),
                dict(n=-1), dict(L=p(lay), mL=p(lmask), n=15), dict(R=ref.data_ptr() + 1), dict(mR=rmask.data_ptr() + 2), dict(L=[lay[0].data_ptr(), lay[1].data_ptr() + 3]),
                dict(mL=[lmask[0].data_ptr() + 1, lmask[1].data_ptr()]), dict(o=out.data_ptr() + 1), dict(k=omask.data_ptr() + 2), dict(v=votes.data_ptr() + 3),
                dict(f=moving.data_ptr() + 2), dict(cnt=counts.data_ptr() + 4), dict(rc=rec.data_ptr() + 4), dict(o=ref.data_ptr()), dict(k=rmask.data_ptr()),
                dict(v=lay[1].data_ptr()), dict(f=lmask[0].data_ptr()), dict(o=rec.data_ptr()), dict(k=out.data_ptr()), dict(v=omask.data_ptr()), dict(f=votes.data_ptr()),
                dict(f=out.data_ptr()), dict(mR=ref.data_ptr()), dict(L=[ref.data_ptr(), lay[1].data_ptr()]), dict(mL=[lay[0].data_ptr(), lmask[1].data_ptr()]),
                dict(mL=[lmask[0].data_ptr(), rmask.data_ptr()]), dict(ch=2), dict(ch=4), dict(r=1), dict(c=16385), dict(r=16385), dict(c=1), dict(th=-1), dict(th=256),
                dict(mv=-1), dict(mv=16), dict(gm=2), dict(gm=-1), dict(mo=-1))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                med(**bad)
        s.synchronize()
        for x in (out, omask, votes, moving):  # nothing was enqueued
            assert (x.cpu().numpy() == GUARD).all()
        assert counts.cpu().numpy().tolist() == [-1] * 6
        for bad in bads[:3]:
            with pytest.raises(rsdsfm.RsdsfmError):
                med(**bad)
            med()  # the same call without the fault goes through
        s.synchronize()
        flat = out.cpu().numpy().reshape(-1)  # candidates 9, 9, 10 in every channel: costs 3, 3, 6 -- the medoid is 9
        assert (flat[:rows * cols * 3] == 9).all() and (flat[rows * cols * 3:] == GUARD).all() and (omask.cpu().numpy().reshape(-1)[:rows * cols] == 1).all()
        assert counts.cpu().numpy().tolist() == [-1, 0, rows * cols, 0, 0, -1] and (votes.cpu().numpy().reshape(-1)[:rows * cols] == 3).all()
        assert (moving.cpu().numpy().reshape(-1)[:rows * cols] == 1).all() and (moving.cpu().numpy().reshape(-1)[rows * cols:] == GUARD).all()
        before = [x.cpu().numpy().copy() for x in (out, omask, votes, moving, counts)]
        for bad in bads:  # a refused call leaves a valid call's outputs as they are
            with pytest.raises(rsdsfm.RsdsfmError):
                med(**bad)
        s.synchronize()
        assert all(np.array_equal(x.cpu().numpy(), b) for x, b in zip((out, omask, votes, moving, counts), before))
        med(L=None, mL=None, n=0, rc=0, v=None, f=None, cnt=None)  # no layers: the arrays and the records may be NULL
        med(L=p(lay[:14]), mL=p(lmask[:14]), n=14)
        s.synchronize()
        # grey candidates 9, 9, 10 .. 22: the medoid is the lower median, index 7 of the ascending order
        assert (votes.cpu().numpy().reshape(-1)[:rows * cols] == 15).all() and (out.cpu().numpy().reshape(-1)[:rows * cols * 3] == 15).all()


# ---------------------------------------------------------------------------------------------------
# the knob
# ---------------------------------------------------------------------------------------------------
def _parts(torch, s, case):
    """the public calls one after another on planes of the test's own, as tests/test_gpu_plate.py makes them, with rsdsfm_plate_medoid_dev in the
    median's place: the own frame's window render (id 1, with a source plane) onto zeroed planes, per neighbour the render alone onto a zeroed
    layer of its own and rsdsfm_seam_overlap_sums_dev into its record, then one rsdsfm_plate_medoid_dev"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case)
    nl = len(src) - 1
    z = lambda like=None: torch.zeros_like(d["frames"][0]) if like is None else torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
    d_ref, d_rm, d_rs = z(), z(1), z(1)
    d_l, d_lm = [z() for _ in range(nl)], [z(1) for _ in range(nl)]
    d_rec = torch.full((8 * max(nl, 1),), -1, dtype=torch.int64, device=dev)
    planes, cnt = _outputs(torch, dev, case["frames"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    kw = dict(mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    arg = lambda k: (d["frames"][src[k]].data_ptr(), ch, d["maps"][src[k]].data_ptr(), d["Rs"][src[k]].data_ptr(), d["ts"][src[k]].data_ptr(), case["K"], rows, cols, M[k], m[k])
    s.stabilize_window_frame_dev(*arg(0), 1, case["window"], d_ref.data_ptr(), d_rm.data_ptr(), d_rs.data_ptr(), **kw)
    for k in range(1, len(src)):
        li, lm = d_l[k - 1].data_ptr(), d_lm[k - 1].data_ptr()
        if case["occlusion"] and case["search"]:
            s.stabilize_search_frame_dev(*arg(k), 2, case["window"], li, lm, tol_q16=case["tol_q16"], **kw)
        elif case["occlusion"]:
            s.stabilize_visible_frame_dev(*arg(k), 2, case["window"], li, lm, tol_q16=case["tol_q16"], **kw)
        else:
            s.stabilize_window_frame_dev(*arg(k), 2, case["window"], li, lm, **kw)
        s.seam_overlap_sums_dev(d_ref.data_ptr(), d_rs.data_ptr(), li, lm, ch, rows, cols, d_rec[8 * (k - 1):].data_ptr())
    s.plate_medoid_dev(d_ref.data_ptr(), d_rm.data_ptr(), [t.data_ptr() for t in d_l], [t.data_ptr() for t in d_lm], ch, rows, cols, planes[0][0].data_ptr(),
                       planes[1][0].data_ptr(), planes[2][0].data_ptr(), planes[3][0].data_ptr(), cnt[1:].data_ptr(), d_rec.data_ptr() if nl else None,
                       min_overlap=case["min_overlap"], gain_mode=case["gain_mode"], threshold=case["threshold"], min_votes=case["min_votes"])
    s.synchronize()
    return _collect(planes, cnt)


def _erase_frame(torch, s, case):
    """one rsdsfm_erase_frame_dev of a case with the mover removal's defaults (open 2, grow 2, feather 4) into guarded, never preset outputs
    -> dict(image, mask, matte, moving, counts (5))"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case)
    planes = [_guarded(torch, dev, np.full(shape, GUARD, dtype=np.uint8)) for shape in (case["frames"][0].shape, (rows, cols), (rows, cols), (rows, cols))]
    cnt = torch.full((7,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s.set_occlusion_search(case["search"])
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    s.erase_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, planes[0][0].data_ptr(), planes[1][0].data_ptr(),
                      planes[2][0].data_ptr(), planes[3][0].data_ptr(), cnt[1:].data_ptr(), **_frame_kw(case))
    s.synchronize()
    s.set_occlusion_search(0)
    assert all((g.cpu().numpy() == GUARD).all() for _, g in planes)
    c = cnt.cpu().numpy().tolist()
    assert c[0] == -1 and c[6] == -1
    return dict({k: p[0].cpu().numpy() for k, p in zip(("image", "mask", "matte", "moving"), planes)}, counts=c[1:6])


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_knob_turns_the_frame_call_to_the_medoid(oracle, rsdsfm, arith):
    """on every case of plate_cases.all_cases: with the knob at 1 plate_frame_dev gives the golden fixture (the definition's plate_frame) and the
    bytes of the public calls made one after another -- the renders, the sums, then rsdsfm_plate_medoid_dev --; erase_frame_dev gives
    erase_spec_numpy's matte and composite on the medoid definition's plate and flag; back at 0 a case gives golden_plate_v1.npz's bytes again; a
    knob value of 2 is refused and changes nothing"""
    import torch

    g, g_median = np.load(GOLDEN), np.load(MEDIAN_GOLDEN)
    with rsdsfm.Solver(0, arith=arith) as s:
        assert s.plate_estimator == 0
        every = cases.all_cases(oracle.pose_table)
        s.set_plate_estimator("medoid")
        assert s.plate_estimator == 1
        for case in every:
            n = case["name"]
            want = _golden(g, n)
            _same(_frame(torch, s, case), want, n)
            s.set_occlusion_search(case["search"])
            parts = _parts(torch, s, case)
            s.set_occlusion_search(0)
            _same(parts, want, n + " parts")
            # the mover removal on this plate
            p = _wanted_frame(case)
            assert np.array_equal(p["image"], want["image"]) and np.array_equal(p["moving"], want["moving"])
            ref, rmask, _ = p["ref"]
            a = erase.matte(p["moving"])
            comp = erase.composite(ref, rmask, p["image"], p["mask"], a)
            got = _erase_frame(torch, s, case)
            assert np.array_equal(got["matte"], a) and np.array_equal(got["moving"], p["moving"]), n
            assert np.array_equal(got["image"], comp["image"]) and np.array_equal(got["mask"], comp["mask"]) and got["counts"] == comp["counts"], n
        for bad in (2, -1, "mean"):
            with pytest.raises(rsdsfm.RsdsfmError):
                s.set_plate_estimator(bad)
            assert s.plate_estimator == 1
        case = {c["name"]: c for c in every}["shift-bgr-0"]
        _same(_frame(torch, s, case), _golden(g, case["name"]), "still the medoid")
        assert not np.array_equal(g[case["name"] + "/image"], g_median[case["name"] + "/image"])  # the case tells the two estimators apart
        s.set_plate_estimator(0)
        _same(_frame(torch, s, case), _golden(g_median, case["name"]), "the median again")
        s.set_plate_estimator(1)
        _same(_frame(torch, s, case), _golden(g, case["name"]), "by number")
        s.set_plate_estimator("median")
        _same(_frame(torch, s, case), _golden(g_median, case["name"]), "by name")
        rows, cols = case["depths"][0].shape
        assert rsdsfm.plate_launches(rows, cols, 5) == 5 * rsdsfm.stabilize_window_launches(rows, cols) + 4 + rsdsfm.plate_medoid_launches()


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_clip_call_follows_the_knob(oracle, rsdsfm, arith):
    """plate_video_dev with the knob at 1: every frame is the frame call's, which is the definition's; a second context is not touched"""
    import torch

    every = {c["name"]: c for c in cases.all_cases(oracle.pose_table)}
    with rsdsfm.Solver(0, arith=arith) as s, rsdsfm.Solver(0, arith=arith) as other:
        s.set_plate_estimator(1)
        for case in (every["gained"], every["shift-bgr-0"]):
            got, d = _video(torch, s, case)
            for q in range(len(case["depths"])):
                want = _wanted_frame(case, q)
                _same(got[q], want, (case["name"], q))
                _same(_frame(torch, s, case, d, q), want, (case["name"], q, "frame"))
        case = every["shift-bgr-0"]
        _same(_frame(torch, other, case), cases.run_spec(case), "the other context's median")
        assert other.plate_estimator == 0


# ---------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_evaluate_real_sequence_with_a_plate_estimator(rsdsfm, tmp_path, arith):
    """evaluate_real_sequence(..., stabilize=True, plate=(1, 30), plate_estimator="medoid") on tests/test_gpu_plate.py's small clip with a mover:
    the keys and files are plate='s, the plates are Solver.plate_video_dev's with the knob at 1 on the clip's own outputs, and the knob is back
    where it was afterwards"""
    import torch

    from test_gpu_stabilize_search import TRIALS, plain_clip

    still, rows, cols, K, gamma, seeds, _ = plain_clip(rsdsfm)
    v, w, k = rsdsfm.synth.default_motion()
    sc = 4.0 / np.abs(rsdsfm.synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)[0]).max()
    frames = [f.copy() for f in rsdsfm.synth.render_sequence(3, rows, cols, K, v * sc, w * sc, k, gamma, seed=21, speeds=(1.0, 1.3), mover=(5, 16, 4, 6, 5, 1))[0]]
    for f in frames:  # the render's channels rise and fall together, so a per-channel median of two candidates is one of them: blue inverted, it is not
        f[..., 0] = 255 - f[..., 0]
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0, plate=(1, 30))
    n = len(frames) - 1
    dev = torch.device("cuda", 0)
    with rsdsfm.Solver(0, arith=arith) as s:
        out = ev(s, frames, plate_estimator="medoid", out_dir=str(tmp_path / "medoid"), **kw)
        assert s.plate_estimator == 0
        plain = ev(s, frames, out_dir=str(tmp_path / "median"), **kw)
        ps, o = out["path_smoothed"], out["pairs"]
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_f, d_z = [tt(frames[q]) for q in range(n)], [tt(np.asarray(o[q]["depth_map"]).T) for q in range(n)]
        d_R, d_t = [tt(np.asarray(o[q]["R"]).reshape(-1, 9)) for q in range(n)], [tt(o[q]["t"]) for q in range(n)]
        outs = [_outputs(torch, dev, frames[0].shape, (rows, cols)) for _ in range(n)]
        torch.cuda.synchronize()
        ptrs = lambda a: [x.data_ptr() for x in a]
        s.set_plate_estimator(1)
        r = s.plate_video_dev(ptrs(d_f), rows, cols, 3, K, ptrs(d_z), ptrs(d_R), ptrs(d_t), out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"],
                              [p[0][0].data_ptr() for p, _ in outs], [p[1][0].data_ptr() for p, _ in outs], None, [p[3][0].data_ptr() for p, _ in outs], radius=1, threshold=30)
        s.synchronize()
        direct = [_collect(p, c, (), False, True, False) for p, c in outs]
    assert set(out) == set(plain)
    assert any(not np.array_equal(out["plate"][p], plain["plate"][p]) for p in range(n))  # the keyword reached the plate
    for p in range(n):
        assert np.array_equal(out["plate"][p], direct[p]["image"]) and np.array_equal(out["plate_moving"][p], direct[p]["moving"])
        assert out["plate_counts"][p].tolist() == r["counts"][p].tolist()
    for k_ in plain:
        if k_ not in ("pairs", "path_smoothed", "links", "plate", "plate_moving", "plate_counts"):
            assert np.asarray(out[k_]).tobytes() == np.asarray(plain[k_]).tobytes(), k_
    assert set(os.listdir(str(tmp_path / "medoid"))) == set(os.listdir(str(tmp_path / "median")))
