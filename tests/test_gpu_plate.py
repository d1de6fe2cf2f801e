"""GPU: the clean plate (include/rsdsfm_plate.h) bit for bit against its definition (tests/plate_spec_numpy.py) in both library builds -- the
median alone at the shapes where its 16 x 64 tile can go wrong and at every layer count where another instance of its kernel runs, the
constructed cases with known answers (the impulse's 3 x 3 footprint across tile borders among them), a seeded random campaign, the frame call
on every case of tests/plate_cases.py against the golden fixture the CPU suite holds to the definition and against the public calls made one
after another, the clip call against the frame calls, the workspace across size changes, argument errors.  Every plane has 16 guard bytes
behind it, the outputs are never preset, the inputs are verified unchanged."""
import functools
import os

import numpy as np
import pytest

import denoise_cases as dcases
import plate_cases as cases
import plate_spec_numpy as spec

pytestmark = pytest.mark.gpu

GUARD = 0xCD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_plate_v1.npz")
PLANES = ("image", "mask", "votes", "moving")


def _guarded(torch, dev, a):
    """a's bytes on the device with 16 guard bytes behind them: (the view of a's shape, the guard)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + 16,), GUARD, dtype=torch.uint8, device=dev)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[:a.size].view(*a.shape), buf[a.size:]


def _outputs(torch, dev, image_shape, plane_shape):
    """the four output planes, never preset (every byte GUARD, and 16 guard bytes behind each), and the counters with a guard on either side"""
    planes = [_guarded(torch, dev, np.full(shape, GUARD, dtype=np.uint8)) for shape in (image_shape, plane_shape, plane_shape, plane_shape)]
    return planes, torch.full((6,), -1, dtype=torch.int64, device=dev)


def _collect(planes, cnt, guards=(), with_votes=True, with_moving=True, with_counts=True):
    for g in [p[1] for p in planes] + list(guards):
        assert (g.cpu().numpy() == GUARD).all()
    c = cnt.cpu().numpy().tolist()
    assert c[0] == -1 and c[5] == -1 and (with_counts or c[1:5] == [-1] * 4)
    out = {k: p[0].cpu().numpy() for k, p in zip(PLANES, planes)}
    assert with_votes or (out["votes"] == GUARD).all()
    assert with_moving or (out["moving"] == GUARD).all()
    return dict(out, counts=c[1:5])


def _same(got, want, name="", votes=True, moving=True, counts=True):
    for k in ("image", "mask") + (("votes",) if votes else ()) + (("moving",) if moving else ()):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert not counts or list(got["counts"]) == list(want["counts"]), (name, got["counts"], want["counts"])


def _median(torch, s, ref, rmask, layers, records=None, with_votes=True, with_moving=True, with_counts=True, **kw):
    """one rsdsfm_plate_median_dev on guarded planes, the outputs never preset -> the collected outputs"""
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
    s.plate_median_dev(d_ref.data_ptr(), d_rm.data_ptr(), [i.data_ptr() for (i, _), _ in d_l], [m.data_ptr() for _, (m, _) in d_l], ch, rows, cols, planes[0][0].data_ptr(),
                       planes[1][0].data_ptr(), planes[2][0].data_ptr() if with_votes else None, planes[3][0].data_ptr() if with_moving else None,
                       cnt[1:].data_ptr() if with_counts else None, d_rec[1:].data_ptr() if d_rec is not None else None, **kw)
    s.synchronize()
    assert np.array_equal(d_ref.cpu().numpy(), ref) and np.array_equal(d_rm.cpu().numpy(), rmask)  # the inputs are only read
    for ((d_i, _), (d_m, _)), (i, m) in zip(d_l, layers):
        assert np.array_equal(d_i.cpu().numpy(), i) and np.array_equal(d_m.cpu().numpy(), m)
    if d_rec is not None:
        assert np.array_equal(d_rec[1:-1].cpu().numpy().view(np.uint64), np.asarray(records, dtype=np.uint64).reshape(-1)) and d_rec[0] == -1 and d_rec[-1] == -1
    guards = [g_ref, g_rm] + [g for (_, gi), (_, gm) in d_l for g in (gi, gm)]
    return _collect(planes, cnt, guards, with_votes, with_moving, with_counts)


def _run_case(torch, s, case, **kw):
    return _median(torch, s, case["ref"], case["rmask"], case["layers"], case["records"], min_overlap=case["min_overlap"], gain_mode=case["gain_mode"],
                   threshold=case["threshold"], min_votes=case["min_votes"], **kw)


# the definition once per input, shared by both builds and never changed
@functools.lru_cache(maxsize=None)
def _wanted(shape, channels, L):
    ref, rmask, ls = cases.median_inputs(shape, channels, L)
    recs = cases.layer_records(channels, L, phase=shape[1])
    threshold, min_votes = cases.median_parameters(shape, L)
    return spec.median(ref, rmask, ls, list(recs), threshold=threshold, min_votes=min_votes)


@functools.lru_cache(maxsize=None)
def _wanted_plain(shape, channels):
    ref, rmask, ls = cases.median_inputs(shape, channels, 2, seed=1)
    recs = cases.layer_records(channels, 2, phase=2)  # both clamps: without the gain they must not show
    return spec.median(ref, rmask, ls, None), spec.median(ref, rmask, ls, list(recs), gain_mode=1, min_overlap=7)


# ---------------------------------------------------------------------------------------------------
# the median
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_median_equals_the_definition(rsdsfm, arith, channels):
    """every shape -- one word, odd sizes, one under, exactly one and one over the tile in both directions, rows that start on every byte of a
    dword, 25 workgroups --; 0, 1, 2, 3, 4, 5, 7, 8, 13 and 14 layers (even and odd numbers of candidates, both ends, and either side of every
    instance of the kernel); masks with empty, full and mixed words and values other than 0 / 1, random bytes under unset mask bytes; the five
    records in turn (both gain clamps, a plain gain, too small an overlap, a layer sum of 0), the gain off, no record; with and without the votes,
    the flag plane and the counters"""
    import torch

    seen = np.zeros(4, dtype=np.int64)
    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in cases.ACC_SHAPES:
            for L in cases.LAYER_COUNTS:
                ref, rmask, ls = cases.median_inputs(shape, channels, L)
                threshold, min_votes = cases.median_parameters(shape, L)
                want = _wanted(shape, channels, L)
                _same(_median(torch, s, ref, rmask, ls, cases.layer_records(channels, L, phase=shape[1]), threshold=threshold, min_votes=min_votes), want, (shape, L))
                seen += np.array(want["counts"])
                if L == 0:
                    on = rmask != 0
                    assert np.array_equal(want["image"], np.where(on if channels == 1 else on[..., None], ref, 0)) and np.array_equal(want["mask"], on)  # the plate is the reference
            ref, rmask, ls = cases.median_inputs(shape, channels, 2, seed=1)
            no_record, gain_off = _wanted_plain(shape, channels)
            _same(_median(torch, s, ref, rmask, ls, None), no_record, (shape, "no record"))
            recs = cases.layer_records(channels, 2, phase=2)
            _same(_median(torch, s, ref, rmask, ls, recs, gain_mode=1, min_overlap=7), gain_off, (shape, "gain off"))
            for votes, moving, counts in ((False, True, True), (True, False, True), (True, True, False), (False, False, False), (True, False, False)):
                _same(_median(torch, s, ref, rmask, ls, recs, votes, moving, counts, gain_mode=1, min_overlap=7), gain_off, shape, votes, moving, counts)
        assert rsdsfm.plate_median_launches() == 1
    assert (seen > 0).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_every_gain(rsdsfm, channels):
    """one layer per record of denoise_cases.records with and without gain_mode 1 and with a min_overlap above the record's count"""
    import torch

    with rsdsfm.Solver(0) as s:
        ref, rmask, ls = cases.median_inputs((33, 129), channels, 1, seed=2)
        for key, r in dcases.records(channels).items():
            for kw in (dict(), dict(gain_mode=1), dict(min_overlap=6000)):
                _same(_median(torch, s, ref, rmask, ls, [r], threshold=60, min_votes=2, **kw), spec.median(ref, rmask, ls, [r], threshold=60, min_votes=2, **kw), (key, kw))


@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_constructed_cases_have_their_known_answers(rsdsfm, arith, channels):
    """tests/plate_cases.constructed on the kernel: all candidates equal, one outlier among fourteen, two candidates, ties, the impulse at every
    corner and edge midpoint of every tile and of the frame at thresholds 1, 24, 40 and 255, min_votes 1 and 15, an empty own mask"""
    import torch

    with rsdsfm.Solver(0, arith=arith) as s:
        for case in cases.constructed(channels):
            got = _run_case(torch, s, case)
            for k, want in case["want"].items():
                assert np.array_equal(np.asarray(got[k]), np.asarray(want)), (case["name"], k)
            assert sum(got["counts"]) == case["rmask"].size


@pytest.mark.parametrize("channels", [1, 3])
def test_the_order_of_the_layers_does_not_matter(rsdsfm, channels):
    import torch

    ref, rmask, ls = cases.median_inputs((37, 67), channels, 5)
    recs = cases.layer_records(channels, 5)
    want = spec.median(ref, rmask, ls, list(recs), threshold=30)
    rng = np.random.default_rng(5)
    with rsdsfm.Solver(0) as s:
        for _ in range(6):
            perm = rng.permutation(5)
            _same(_median(torch, s, ref, rmask, [ls[i] for i in perm], recs[perm], threshold=30), want, perm.tolist())


def test_a_seeded_random_campaign(rsdsfm):
    """200 small cases: shapes up to 40 x 140, 0 .. 14 layers, sparse to dense masks, records or none, every parameter"""
    import torch

    rng = np.random.default_rng(20240)
    layer_counts = set()
    with rsdsfm.Solver(0) as s:
        for k in range(200):
            case = cases.random_case(rng)
            _same(_run_case(torch, s, case), cases.spec_of(case), (k, case["ref"].shape, len(case["layers"])))
            layer_counts.add(len(case["layers"]))
    assert layer_counts == set(range(15))


def test_the_host_convenience_of_the_median(rsdsfm):
    ref, rmask, ls = cases.median_inputs((37, 67), 3, 3)
    recs = cases.layer_records(3, 3)
    with rsdsfm.Solver(0) as s:
        img, mask, votes, moving, counts = s.plate_median(ref, rmask, ls, recs, threshold=30)
        _same(dict(image=img, mask=mask, votes=votes, moving=moving, counts=counts.tolist()), spec.median(ref, rmask, ls, list(recs), threshold=30))
        img, mask, votes, moving, counts = s.plate_median(ref, rmask, [])
        _same(dict(image=img, mask=mask, votes=votes, moving=moving, counts=counts.tolist()), spec.median(ref, rmask, []))


def test_median_argument_errors(rsdsfm):
    """every refusal returns RSDSFM_ERR_INVALID and enqueues nothing: the outputs keep their sentinel; after a refused call the same call without
    the fault goes through"""
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
    with rsdsfm.Solver(0) as s:
        def med(R=ref.data_ptr(), mR=rmask.data_ptr(), L=p(lay[:2]), mL=p(lmask[:2]), n=None, ch=3, r=rows, c=cols, rc=rec.data_ptr(), mo=0, gm=0, th=24, mv=3,
                o=out.data_ptr(), k=omask.data_ptr(), v=votes.data_ptr(), f=moving.data_ptr(), cnt=counts[1:].data_ptr()):
            return s.plate_median_dev(R, mR, L, mL, ch, r, c, o, k, v, f, cnt, rc, mo, gm, th, mv, nlayers=n)

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
        flat = out.cpu().numpy().reshape(-1)  # candidates 9, 9, 10: the lower median is 9
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
        assert (votes.cpu().numpy().reshape(-1)[:rows * cols] == 15).all() and (out.cpu().numpy().reshape(-1)[:rows * cols * 3] == 15).all()  # 9, 9 .. 22: index 7


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
def _clip(torch, dev, case):
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(frames=[tt(x) for x in case["frames"]], maps=[tt(z.T) for z in case["depths"]], Rs=[tt(np.asarray(R).reshape(-1, 9)) for R in case["Rs"]],
                ts=[tt(t) for t in case["ts"]])


def _frame_kw(case):
    return dict(threshold=case["threshold"], min_votes=case["min_votes"], gain=case["gain_mode"] == 0, min_overlap=case["min_overlap"], window=case["window"],
                occlusion=case["occlusion"], occlusion_tol_q16=case["tol_q16"], mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])


def _frame(torch, s, case, d=None, q=None, with_votes=True, with_moving=True, with_counts=True):
    """one rsdsfm_plate_frame_dev of frame q of a case (the context's knob set to the case's) into guarded, never preset outputs"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    d = d or _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case, q)
    planes, cnt = _outputs(torch, dev, case["frames"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    s.set_occlusion_search(case["search"])
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    s.plate_frame_dev(pick("frames"), ch, pick("maps"), pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, planes[0][0].data_ptr(), planes[1][0].data_ptr(),
                      planes[2][0].data_ptr() if with_votes else None, planes[3][0].data_ptr() if with_moving else None, cnt[1:].data_ptr() if with_counts else None,
                      **_frame_kw(case))
    s.synchronize()
    s.set_occlusion_search(0)
    for t, a in zip(d["frames"], case["frames"]):
        assert np.array_equal(t.cpu().numpy(), a)
    return _collect(planes, cnt, (), with_votes, with_moving, with_counts)


def _parts(torch, s, case):
    """the public calls one after another on planes of the test's own: the own frame's window render (id 1, with a source plane) onto zeroed
    planes, then per neighbour the render alone onto a zeroed layer of its own and rsdsfm_seam_overlap_sums_dev into its record, then one
    rsdsfm_plate_median_dev"""
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
    s.plate_median_dev(d_ref.data_ptr(), d_rm.data_ptr(), [t.data_ptr() for t in d_l], [t.data_ptr() for t in d_lm], ch, rows, cols, planes[0][0].data_ptr(),
                       planes[1][0].data_ptr(), planes[2][0].data_ptr(), planes[3][0].data_ptr(), cnt[1:].data_ptr(), d_rec.data_ptr() if nl else None,
                       min_overlap=case["min_overlap"], gain_mode=case["gain_mode"], threshold=case["threshold"], min_votes=case["min_votes"])
    s.synchronize()
    return _collect(planes, cnt), dict(image=d_ref.cpu().numpy(), mask=d_rm.cpu().numpy())


def _golden(g, name):
    return dict({k: g[name + "/" + k] for k in PLANES}, counts=g[name + "/counts"].tolist())


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_every_case_equals_the_definition_and_the_public_calls(oracle, rsdsfm, arith):
    """plate, mask, votes, flag plane and the four counts of every fixture case -- the noisy shift scene gray and BGR, a fold pair plain, through
    the occlusion test and through the search, a zoomed window, gained neighbours with the gain on, off and under too small an overlap, five
    sources from the clip's middle, one-sided and at radius 7, one source, the 2 x 2 dense case -- against the golden fixture (the definition's
    plate_frame), and against the public calls made one after another; the launch count; one source alone is the window render.  The cases
    change the frame size again and again on ONE context: the workspace is released and regrown, and grows with the number of neighbours"""
    import torch

    g = np.load(GOLDEN)
    with rsdsfm.Solver(0, arith=arith) as s:
        every = cases.all_cases(oracle.pose_table)
        for case in every:
            n = case["name"]
            want = _golden(g, n)
            _same(_frame(torch, s, case), want, n)
            s.set_occlusion_search(case["search"])
            parts, ref = _parts(torch, s, case)
            s.set_occlusion_search(0)
            _same(parts, want, n + " parts")
            nsrc = len(dcases.sources_and_poses(case)[0])
            if nsrc == 1:
                assert np.array_equal(want["image"], ref["image"]) and np.array_equal(want["mask"], ref["mask"])
            rows, cols = case["depths"][0].shape
            assert rsdsfm.plate_launches(rows, cols, nsrc) == nsrc * rsdsfm.stabilize_window_launches(rows, cols) + (nsrc - 1) + rsdsfm.plate_median_launches()
        # fewer neighbours after more, the same size: the larger stack is kept; then back to a size seen before
        by_name = {c["name"]: c for c in every}
        for n in ("five-middle", "five-first", "five-middle", "gained", "2x2", "five-radius-7"):
            _same(_frame(torch, s, by_name[n]), _golden(g, n), n + " again")
        case = every[0]
        want = cases.run_spec(case)
        for votes, moving, counts in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            _same(_frame(torch, s, case, with_votes=votes, with_moving=moving, with_counts=counts), want, "optional outputs", votes, moving, counts)


def test_the_mover_scene_on_the_gpu(rsdsfm):
    """the scene of tests/test_plate_cpu.py's quality test through the frame call: the definition's bytes"""
    import torch

    case, _ = cases.mover_scene()
    with rsdsfm.Solver(0) as s:
        got = _frame(torch, s, case)
    _same(got, cases.run_spec(case), "mover")
    assert got["counts"][2] > 0


def test_frame_argument_errors(oracle, rsdsfm):
    """a refused frame call enqueues nothing: the outputs keep their guard bytes"""
    import torch

    dev = torch.device("cuda", 0)
    case = [c for c in cases.all_cases(oracle.pose_table) if c["name"] == "gained"][0]
    rows, cols = case["depths"][0].shape
    d = _clip(torch, dev, case)
    src, M, m = dcases.sources_and_poses(case)
    planes, cnt = _outputs(torch, dev, case["frames"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    pick = lambda k: [d[k][n].data_ptr() for n in src]
    with rsdsfm.Solver(0) as s:
        def call(images=pick("frames"), maps=pick("maps"), M=M, m=m, o=planes[0][0].data_ptr(), k=planes[1][0].data_ptr(), v=planes[2][0].data_ptr(), f=planes[3][0].data_ptr(),
                 cnt_=cnt[1:].data_ptr(), ch=3, **kw):
            return s.plate_frame_dev(images, ch, maps, pick("Rs"), pick("ts"), case["K"], rows, cols, M, m, o, k, v, f, cnt_, **kw)

        bad_M = M.copy()
        bad_M[1, 0, 0] = np.nan
        params = rsdsfm.PlateParams()
        params.struct_bytes = 40
        bads = (dict(images=[0] + pick("frames")[1:]), dict(maps=pick("maps")[:2] + [0]), dict(images=[]),
                dict(images=pick("frames") * 6, maps=pick("maps") * 6, M=np.tile(M, (6, 1, 1)), m=np.tile(m, (6, 1))), dict(M=bad_M), dict(o=0), dict(k=0),
                dict(o=planes[1][0].data_ptr()), dict(v=planes[0][0].data_ptr()), dict(f=planes[2][0].data_ptr()), dict(o=planes[0][0].data_ptr() + 1),
                dict(f=planes[3][0].data_ptr() + 2), dict(cnt_=cnt.data_ptr() + 4), dict(o=pick("frames")[2]), dict(f=pick("frames")[1]), dict(ch=2), dict(threshold=256),
                dict(threshold=-1), dict(min_votes=16), dict(min_votes=-1), dict(min_overlap=-1), dict(occlusion=2), dict(occlusion=True, occlusion_tol_q16=65537),
                dict(window=(0, 0, rows + 1, cols)), dict(window=(1, 1, 0, 4)), dict(iterations=17), dict(params=params))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        for (p, gd) in planes:
            assert (p.cpu().numpy() == GUARD).all() and (gd.cpu().numpy() == GUARD).all()
        assert cnt.cpu().numpy().tolist() == [-1] * 6
        call(threshold=case["threshold"], min_votes=case["min_votes"])
        s.synchronize()
        _same(_collect(planes, cnt), cases.run_spec(case))


# ---------------------------------------------------------------------------------------------------
# the clip call
# ---------------------------------------------------------------------------------------------------
def _video(torch, s, case, want_counts=True, with_optional=True):
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    ns = len(case["depths"])
    d = _clip(torch, dev, case)
    outs = [_outputs(torch, dev, case["frames"][0].shape, (rows, cols)) for _ in range(ns)]
    torch.cuda.synchronize()
    ptrs = lambda a: [x.data_ptr() for x in a]
    s.set_occlusion_search(case["search"])
    r = s.plate_video_dev(ptrs(d["frames"]), rows, cols, ch, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"], case["c_path"],
                          case["scales"], [p[0][0].data_ptr() for p, _ in outs], [p[1][0].data_ptr() for p, _ in outs],
                          [p[2][0].data_ptr() for p, _ in outs] if with_optional else None, [p[3][0].data_ptr() for p, _ in outs] if with_optional else None,
                          want_counts=want_counts, radius=case["radius"], **_frame_kw(case))
    s.synchronize()
    s.set_occlusion_search(0)
    got = []
    for q, (planes, cnt) in enumerate(outs):
        one = _collect(planes, cnt, (), with_optional, with_optional, False)
        one["counts"] = r["counts"][q].tolist() if want_counts else None
        got.append(one)
    return got, d


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_clip_call_equals_the_frame_calls(oracle, rsdsfm, arith):
    """three sources (radius 1) and five (radius 2, the first and last frames with one-sided neighbours; the noisy shift scene, whose path is the
    chain itself, and a smooth clip on a path of its own) and one source alone: every frame of the clip call is the frame call's, which is the
    definition's; without the counters, the votes and the flag planes the call only enqueues"""
    import torch

    every = {c["name"]: c for c in cases.all_cases(oracle.pose_table)}
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in (every["gained"], every["five-middle"], every["shift-bgr-0"], every["one-source"], dict(every["fold-search"], radius=2)):
            got, d = _video(torch, s, case)
            ns = len(case["depths"])
            for q in range(ns):
                want = cases.run_spec(case, q)
                _same(got[q], want, (case["name"], q))
                _same(_frame(torch, s, case, d, q), want, (case["name"], q, "frame"))
            if ns == 5:
                assert [len(dcases.sources_and_poses(case, q)[0]) for q in range(5)] == [3, 4, 5, 4, 3]
        case = every["five-middle"]
        got, _ = _video(torch, s, case, want_counts=False, with_optional=False)
        for q in range(5):
            _same(got[q], cases.run_spec(case, q), q, votes=False, moving=False, counts=False)
        # a refused clip call enqueues nothing
        dev = torch.device("cuda", 0)
        rows, cols = case["depths"][0].shape
        d = _clip(torch, dev, case)
        outs = [_outputs(torch, dev, case["frames"][0].shape, (rows, cols)) for _ in range(5)]
        torch.cuda.synchronize()
        ptrs = lambda a: [x.data_ptr() for x in a]
        bad_scales = case["scales"].copy()
        bad_scales[4] = 0.0

        def call(scales=case["scales"], o=None, f=None, **kw):
            return s.plate_video_dev(ptrs(d["frames"]), rows, cols, 1, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"], case["A_path"],
                                     case["c_path"], scales, o or [p[0][0].data_ptr() for p, _ in outs], [p[1][0].data_ptr() for p, _ in outs], None, f, **kw)

        for bad in (dict(scales=bad_scales), dict(radius=8), dict(radius=-1), dict(threshold=300), dict(min_votes=16), dict(o=[outs[0][0][0][0].data_ptr()] * 4 + [0]),
                    dict(o=[outs[0][0][0][0].data_ptr()] * 4 + [d["frames"][1].data_ptr()]), dict(f=[outs[0][0][3][0].data_ptr()] * 4 + [0])):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        s.synchronize()
        for planes, _ in outs:
            for p, gd in planes:
                assert (p.cpu().numpy() == GUARD).all() and (gd.cpu().numpy() == GUARD).all()


# ---------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------
def test_evaluate_real_sequence_with_plate(rsdsfm, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, plate=K or (K, threshold)) on a small synthetic clip with a mover adds exactly plate, plate_moving
    and plate_counts and the files plate_<p>.png, moving_<p>.png and plate.csv, and the arrays are Solver.plate_video_dev's on the clip's own
    outputs; without the keyword every key and file is what it was"""
    import torch

    from test_gpu_stabilize_search import TRIALS, plain_clip

    still, rows, cols, K, gamma, seeds, _ = plain_clip(rsdsfm)
    v, w, k = rsdsfm.synth.default_motion()
    sc = 4.0 / np.abs(rsdsfm.synth.make_flow(rows, cols, K, v, w, k, gamma, _model_only=True)[0]).max()
    mover = (5, 16, 4, 6, 5, 1)  # plain_clip's render with something that moves through the static scene
    frames = rsdsfm.synth.render_sequence(3, rows, cols, K, v * sc, w * sc, k, gamma, seed=21, speeds=(1.0, 1.3), mover=mover)[0]
    planes = rsdsfm.synth.mover_planes(3, rows, cols, mover)
    assert all(np.array_equal(frames[j][~planes[j]], still[j][~planes[j]]) and not np.array_equal(frames[j], still[j]) for j in range(3))
    frames = list(frames)
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
    n = len(frames) - 1
    dev = torch.device("cuda", 0)
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, plate=(1, 30), out_dir=str(tmp_path / "with"), **kw)
        plain = ev(s, frames, out_dir=str(tmp_path / "without"), **kw)
        default = ev(s, frames, plate=2, **kw)
        ps, o = out["path_smoothed"], out["pairs"]
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_f, d_z = [tt(frames[q]) for q in range(n)], [tt(np.asarray(o[q]["depth_map"]).T) for q in range(n)]
        d_R, d_t = [tt(np.asarray(o[q]["R"]).reshape(-1, 9)) for q in range(n)], [tt(o[q]["t"]) for q in range(n)]
        outs = [_outputs(torch, dev, frames[0].shape, (rows, cols)) for _ in range(n)]
        torch.cuda.synchronize()
        ptrs = lambda a: [x.data_ptr() for x in a]
        r = s.plate_video_dev(ptrs(d_f), rows, cols, 3, K, ptrs(d_z), ptrs(d_R), ptrs(d_t), out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"],
                              [p[0][0].data_ptr() for p, _ in outs], [p[1][0].data_ptr() for p, _ in outs], None, [p[3][0].data_ptr() for p, _ in outs], radius=1, threshold=30)
        s.synchronize()
        direct = [_collect(p, c, (), False, True, False) for p, c in outs]
    new = {"plate", "plate_moving", "plate_counts"}
    assert set(out) == set(plain) | new == set(default)
    assert len(out["plate"]) == len(out["plate_moving"]) == n and out["plate_counts"].shape == (n, 4)
    for p in range(n):
        assert np.array_equal(out["plate"][p], direct[p]["image"]) and np.array_equal(out["plate_moving"][p], direct[p]["moving"])
        assert out["plate_counts"][p].tolist() == r["counts"][p].tolist() and out["plate_counts"][p].sum() == rows * cols
        assert out["plate"][p].shape == frames[0].shape and [int((out["plate_moving"][p] == k).sum()) for k in range(4)] == out["plate_counts"][p].tolist()
    for k in plain:
        if k not in ("pairs", "path_smoothed", "links"):
            assert np.asarray(out[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    with_files, without_files = set(os.listdir(str(tmp_path / "with"))), set(os.listdir(str(tmp_path / "without")))
    assert with_files == without_files | {"plate_%d.png" % p for p in range(n)} | {"moving_%d.png" % p for p in range(n)} | {"plate.csv"}
    lines = open(str(tmp_path / "with" / "plate.csv")).read().split()
    assert lines[0] == "pair,unset,static,moving,undecided" and len(lines) == 1 + n
    assert lines[1].split(",") == ["0"] + [str(int(x)) for x in out["plate_counts"][0]]
