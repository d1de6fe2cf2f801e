"""GPU: one candidate of the border fill (rsdsfm_stabilize_fill_frame_dev) bit for bit against its definition
(tests/stabilize_fill_spec_numpy.py: fill_from) -- image, mask, source plane and the filled count --, the starting masks that drive the
kernel's three paths, the two exact cases, the optional outputs and argument errors; and the clip call
(rsdsfm_stabilize_video_filled_dev) byte for byte against the public calls made one after another.  Inputs as
tests/test_gpu_stabilize.py's (tests/stabilize_fill_cases.py)."""
import numpy as np
import pytest

import link_spec_numpy as link
import rectify_dense_spec_numpy as dense
import stabilize_cases as stab_cases
import stabilize_fill_cases as cases
import stabilize_fill_spec_numpy as spec
import stabilize_spec_numpy as stab
from test_gpu_video import _buffers, _record, _scaled_motion

pytestmark = pytest.mark.gpu

# the neighbour's pose in the own frame's virtual camera: another rotation and a baseline in the pair's unit (depths are 0.6 .. 2.5), chosen so
# that it covers a good part of the band the own frame leaves (346 of 792 pixels at 96 x 128)
M_N = link.rodrigues(np.array([-0.03, 0.04, -0.02]))
m_N = np.array([-0.1, 0.05, -0.15])
SID = 2
GUARD = 0xCD

HOLES = dict(holes=0.4)
SHAPES = [(2, 2),     # the whole frame in the byte tail
          (3, 5),     # 15 pixels: three whole words and the byte tail
          (24, 40),
          (33, 70),   # ragged tiles, the byte tail
          (96, 128)]  # several tiles and workgroups
CASES = [(shape, ch, 0, 0, 0, "reference", HOLES) for shape in SHAPES for ch in (3, 1)]
CASES += [((33, 70), 3, it, 0, 0, "reference", HOLES) for it in (1, 3)]
CASES += [((33, 70), 3, 0, mode, q5, "reference", HOLES) for mode, q5 in ((0, 1), (1, 0))]
CASES += [((33, 70), 3, 0, 0, 0, "fused", HOLES), ((96, 128), 1, 0, 0, 0, "fused", HOLES)]
CASES += [((33, 70), 3, 0, 0, 0, "reference", dict(holes=0.4, specials=True)),                      # NaN, +-inf, negative and 1e308 depths
          ((33, 70), 1, 0, 0, 0, "reference", dict(holes=0.7, block=(8, 20, 10, 14), corner=(5, 9)))]  # a thinner map

_expected = {}


def _pair(oracle, shape, ch, it, mode, q5, nkw):
    """an own frame (the stabiliser's standard case) and a neighbour of other bytes and other holes, with the spec's own frame and candidate,
    computed once per case and shared"""
    key = (shape, ch, it, mode, q5, tuple(sorted(nkw.items())))
    if key not in _expected:
        rows, cols = shape
        K, image, depth = cases.inputs(rows, cols, channels=ch, holes=0.4)
        _, _, ndepth = cases.inputs(rows, cols, channels=ch, **nkw)
        R, t = oracle.pose_table(cases.POSE["v"], cases.POSE["w"], cases.POSE["k"], cases.POSE["gamma"], rows)
        R = np.ascontiguousarray(R).reshape(rows, 9)
        nimage = np.ascontiguousarray(np.roll(image, (1, 2), axis=(0, 1))[::-1])
        ndepth = np.ascontiguousarray(np.roll(ndepth, (1, 2), axis=(0, 1)))
        own = stab.stabilize_frame(image, depth, R, t, K, stab_cases.M_STD, stab_cases.m_STD, mode=mode, q5_mode=q5, iterations=it)
        cand = stab.stabilize_frame(nimage, ndepth, R, t, K, M_N, m_N, mode=mode, q5_mode=q5, iterations=it)
        _expected[key] = dict(K=K, image=image, depth=depth, R=R, t=t, nimage=nimage, ndepth=ndepth, own=own, cand=cand)
    return _expected[key]


def _want(e, image, mask, source):
    """fill_from's result on these planes, from the case's candidate (the candidate does not depend on them)"""
    take = (mask == 0) & (e["cand"]["mask"] == 1)
    out, m2, s2 = image.copy(), mask.copy(), source.copy()
    out[take] = e["cand"]["image"][take]
    m2[take] = 1
    s2[take] = SID
    return dict(image=out, mask=m2, source=s2, count=int(take.sum()))


def _guarded(torch, dev, a):
    """a's bytes on the device with 16 guard bytes behind them: (the view of a's shape, the guard)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + 16,), GUARD, dtype=torch.uint8, device=dev)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[:a.size].view(*a.shape), buf[a.size:]


def _fill(torch, s, e, image, mask, source, it=0, mode=0, q5=0, nimage=None, ndepth=None, M=M_N, m=m_N, sid=SID, with_source=True, with_count=True):
    """one fill call on the given in-out planes (host arrays); every plane has guard bytes behind it and the counter a guard on either side"""
    dev = torch.device("cuda", 0)
    rows, cols = mask.shape
    ch = 1 if image.ndim == 2 else 3
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_n, d_dm = tt(e["nimage"] if nimage is None else nimage), tt((e["ndepth"] if ndepth is None else ndepth).T)
    d_R, d_t = tt(e["R"]), tt(e["t"])
    (d_img, g_img), (d_mask, g_mask), (d_src, g_src) = _guarded(torch, dev, image), _guarded(torch, dev, mask), _guarded(torch, dev, source)
    cnt = torch.full((3,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s.stabilize_fill_frame_dev(d_n.data_ptr(), ch, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, M, m, sid, d_img.data_ptr(), d_mask.data_ptr(),
                               d_src.data_ptr() if with_source else None, cnt[1:].data_ptr() if with_count else None, mode=mode, q5_mode=q5, iterations=it)
    s.synchronize()
    for g in (g_img, g_mask, g_src):
        assert (g.cpu().numpy() == GUARD).all()
    c = cnt.cpu().numpy().tolist()
    assert c[0] == -1 and c[2] == -1
    return dict(image=d_img.cpu().numpy(), mask=d_mask.cpu().numpy(), source=d_src.cpu().numpy(), count=c[1])


def _same(got, want):
    for k in ("image", "mask", "source"):
        assert np.array_equal(got[k], want[k]), k
    assert got["count"] == want["count"]


def _own_on_device(torch, s, e, it, mode, q5):
    """the in-out planes from a real own call"""
    dev = torch.device("cuda", 0)
    rows, cols = e["depth"].shape
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_img, d_dm, d_R, d_t = tt(e["image"]), tt(e["depth"].T), tt(e["R"]), tt(e["t"])
    out, mask = torch.full_like(d_img, 77), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s.stabilize_frame_dev(d_img.data_ptr(), 1 if e["image"].ndim == 2 else 3, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, stab_cases.M_STD,
                          stab_cases.m_STD, out.data_ptr(), mask.data_ptr(), mode=mode, q5_mode=q5, iterations=it)
    s.synchronize()
    return out.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.parametrize("shape,ch,it,mode,q5,arith,nkw", CASES)
def test_fill_call_equals_fill_from(oracle, rsdsfm, shape, ch, it, mode, q5, arith, nkw):
    import torch

    e = _pair(oracle, shape, ch, it, mode, q5, nkw)
    assert rsdsfm.stabilize_fill_launches(*shape) == rsdsfm.rectify_dense_launches(*shape)
    with rsdsfm.Solver(0, arith=arith) as s:
        image, mask = _own_on_device(torch, s, e, it, mode, q5)
        assert np.array_equal(image, e["own"]["image"]) and np.array_equal(mask, e["own"]["mask"])
        want = _want(e, image, mask, mask)
        if shape[0] * shape[1] > 900 and mode == 0:
            assert 0 < want["count"] < (mask == 0).sum()  # something is filled, something is left
        _same(_fill(torch, s, e, image, mask, mask, it, mode, q5), want)


@pytest.mark.parametrize("shape,ch", [((3, 5), 3), ((33, 70), 3), ((33, 70), 1), ((24, 40), 1)])
def test_starting_masks(oracle, rsdsfm, shape, ch):
    """all 1: no byte changes and the count is 0 (the early exit); all 0: the candidate's stabilised frame exactly (no read of the image); every
    pattern of the 4 bytes of a word: the read-modify-write path"""
    import torch

    e = _pair(oracle, shape, ch, 0, 0, 0, HOLES)
    rows, cols = shape
    rng = np.random.default_rng(5)
    image = rng.integers(0, 256, size=e["image"].shape, dtype=np.uint8)
    source = rng.integers(6, 200, size=shape, dtype=np.uint8)
    pattern = ((np.arange(rows * cols) // 4 % 16) >> (np.arange(rows * cols) % 4) & 1).astype(np.uint8).reshape(shape)
    assert rows * cols < 64 or len({tuple(w) for w in pattern.reshape(-1)[:64].reshape(16, 4)}) == 16
    with rsdsfm.Solver(0) as s:
        ones = _fill(torch, s, e, image, np.ones(shape, dtype=np.uint8), source)
        assert np.array_equal(ones["image"], image) and ones["mask"].all() and np.array_equal(ones["source"], source) and ones["count"] == 0
        zeros = _fill(torch, s, e, image, np.zeros(shape, dtype=np.uint8), source)
        cm = e["cand"]["mask"] == 1
        assert np.array_equal(zeros["mask"], e["cand"]["mask"]) and zeros["count"] == int(cm.sum())
        assert np.array_equal(zeros["image"][cm], e["cand"]["image"][cm]) and np.array_equal(zeros["image"][~cm], image[~cm])
        assert (zeros["source"][cm] == SID).all() and np.array_equal(zeros["source"][~cm], source[~cm])
        blank = _fill(torch, s, e, np.zeros_like(image), np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8))
        assert np.array_equal(blank["image"], e["cand"]["image"]) and np.array_equal(blank["source"], SID * e["cand"]["mask"])
        _same(_fill(torch, s, e, image, pattern, source), _want(e, image, pattern, source))
        _same(_fill(torch, s, e, image, 1 - pattern, source), _want(e, image, 1 - pattern, source))
    if rows * cols > 900:
        assert 0 < _want(e, image, pattern, source)["count"] < (pattern == 0).sum()


def test_exact_cases_on_the_device(rsdsfm):
    import torch

    c = cases.shift_fill_case()
    e = dict(c, nimage=c["neighbour"], ndepth=c["depth"])
    with rsdsfm.Solver(0) as s:
        for name in ("full", "partial"):
            x = c[name]
            got = _fill(torch, s, e, c["want"], c["mask"], c["mask"], M=x["M"], m=x["m"])
            assert np.array_equal(got["image"], x["want"]) and np.array_equal(got["mask"] == 1, (c["mask"] == 1) | x["take"])
            assert np.array_equal(got["source"], c["mask"] + 2 * x["take"].astype(np.uint8))
            assert (got["mask"].size - 640 - got["count"], 640, got["count"]) == x["counts"]
            # the host convenience on a clip of two pairs whose poses give exactly (M, m): frame 1 is the NEXT frame, source id 3
            A, cc = np.stack([np.eye(3)] * 3), np.stack([np.zeros(3), x["m"] - c["m"], np.zeros(3)])
            As, cs = A.copy(), np.stack([-c["m"], cc[1], np.zeros(3)])
            img, mask, source, counts = s.stabilize_filled([c["image"], c["neighbour"]], [c["depth"]] * 2, [c["R"]] * 2, [c["t"]] * 2, c["K"], A, cc, As, cs, np.ones(2),
                                                           0, c["M"], c["m"], radius=1)
            assert np.array_equal(img, x["want"]) and np.array_equal(source, c["mask"] + 3 * x["take"].astype(np.uint8)) and np.array_equal(mask, got["mask"])
            assert counts.tolist() == [x["counts"][0], 640, 0, x["counts"][2]]


def test_a_candidate_without_a_valid_depth_changes_nothing(oracle, rsdsfm):
    import torch

    e = _pair(oracle, (33, 70), 3, 0, 0, 0, HOLES)
    _, _, none_valid = cases.inputs(33, 70, none_valid=True)
    image, mask = e["own"]["image"], e["own"]["mask"]
    with rsdsfm.Solver(0) as s:
        got = _fill(torch, s, e, image, mask, mask, ndepth=none_valid)
    assert np.array_equal(got["image"], image) and np.array_equal(got["mask"], mask) and np.array_equal(got["source"], mask) and got["count"] == 0


@pytest.mark.parametrize("ch,q,radius", [(3, 2, 2), (1, 1, 2), (3, 2, 1)])
def test_neighbours_in_sequence_follow_the_specs_precedence(oracle, rsdsfm, ch, q, radius):
    """Solver.stabilize_filled: the own call and one fill call per candidate, against stabilize_filled_frame"""
    cc = cases.clip_case(oracle.pose_table, 33, 70, channels=ch)
    want = spec.stabilize_filled_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], q, cc["M"][q],
                                       cc["m"][q], radius=radius)
    with rsdsfm.Solver(0) as s:
        img, mask, source, counts = s.stabilize_filled(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], q,
                                                       cc["M"][q], cc["m"][q], radius=radius)
    assert np.array_equal(img, want["image"]) and np.array_equal(mask, want["mask"]) and np.array_equal(source, want["source"])
    assert counts.tolist() == want["counts"] and sum(1 for x in want["counts"][2:] if x) >= 2  # more than one neighbour gave something


def test_outputs_are_optional_and_nothing_else_is_written(oracle, rsdsfm):
    import torch

    e = _pair(oracle, (33, 70), 3, 0, 0, 0, HOLES)
    image, mask = e["own"]["image"], e["own"]["mask"]
    untouched = np.full(mask.shape, GUARD, dtype=np.uint8)
    want = _want(e, image, mask, mask)
    with rsdsfm.Solver(0) as s:
        for with_source, with_count in ((False, False), (False, True), (True, False)):
            got = _fill(torch, s, e, image, mask, mask if with_source else untouched, with_source=with_source, with_count=with_count)
            assert np.array_equal(got["image"], want["image"]) and np.array_equal(got["mask"], want["mask"])
            assert np.array_equal(got["source"], want["source"] if with_source else untouched)
            assert got["count"] == (want["count"] if with_count else -1)


def test_argument_errors(rsdsfm):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    img = torch.zeros((rows, cols, 3), dtype=torch.uint8, device=dev)
    out = torch.zeros_like(img)
    mask, source = torch.zeros((rows, cols + 4), dtype=torch.uint8, device=dev), torch.zeros((rows, cols + 4), dtype=torch.uint8, device=dev)
    filled = torch.zeros(2, dtype=torch.int64, device=dev)
    dm, t = torch.ones(rows * cols, dtype=torch.float64, device=dev), torch.zeros(rows * 3, dtype=torch.float64, device=dev)
    R = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 9).repeat(rows, 1).contiguous()
    K = (50.0, 50.0, 32.0, 8.0)
    nanM, infm = np.eye(3), np.zeros(3)
    nanM[1, 2], infm[0] = np.nan, np.inf
    with rsdsfm.Solver(0) as s:
        call = lambda i=img.data_ptr(), ch=3, d=dm.data_ptr(), o=out.data_ptr(), r=rows, c=cols, M=np.eye(3), m=np.zeros(3), sid=2, k=mask.data_ptr(), **kw: \
            s.stabilize_fill_frame_dev(i, ch, d, R.data_ptr(), t.data_ptr(), K, r, c, M, m, sid, o, k, **kw)
        for bad in (dict(M=None), dict(m=None), dict(M=nanM), dict(m=infm),
                    dict(o=img.data_ptr()),  # the neighbour's image is the in-out image
                    dict(d_source=mask.data_ptr()),  # the source plane is the mask
                    dict(o=0), dict(i=0), dict(d=0), dict(k=0), dict(ch=2), dict(mode=2), dict(q5_mode=7), dict(iterations=17), dict(iterations=-1),
                    dict(r=1), dict(c=1), dict(c=16385), dict(sid=1), dict(sid=0), dict(sid=256), dict(sid=-3),
                    dict(o=out.data_ptr() + 1), dict(i=img.data_ptr() + 2), dict(k=mask.data_ptr() + 2), dict(d_source=source.data_ptr() + 1),
                    dict(d_filled=filled.data_ptr() + 4)):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        call(sid=255, d_source=source.data_ptr(), d_filled=filled.data_ptr())  # the same arguments without a fault go through
        s.synchronize()
    assert int(filled.cpu()[0]) == rows * cols  # constant depth, identity poses: every pixel of the empty mask is taken


def test_dense_stabilise_and_fill_alternate_on_one_context(oracle, rsdsfm):
    """dense, stabilise and fill calls at two sizes on ONE context (one workspace, rebuilt only when the size changes): the spec's result every
    time"""
    import torch

    dev = torch.device("cuda", 0)
    a, b = _pair(oracle, (33, 70), 3, 0, 0, 0, HOLES), _pair(oracle, (96, 128), 1, 0, 0, 0, HOLES)
    want_dense = {id(e): dense.rectify_dense(e["image"], e["depth"], e["R"], e["t"], *e["K"]) for e in (a, b)}
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def dense_call(s, e):
        rows, cols = e["depth"].shape
        d_img, d_dm, d_R, d_t = tt(e["image"]), tt(e["depth"].T), tt(e["R"]), tt(e["t"])
        out, mask = torch.full_like(d_img, 77), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        s.rectify_dense_frame_dev(d_img.data_ptr(), 1 if e["image"].ndim == 2 else 3, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, out.data_ptr(),
                                  mask.data_ptr())
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), want_dense[id(e)]["image"]) and np.array_equal(mask.cpu().numpy(), want_dense[id(e)]["mask"])

    with rsdsfm.Solver(0) as s:
        for e in (a, b, a):
            dense_call(s, e)
            image, mask = _own_on_device(torch, s, e, 0, 0, 0)
            assert np.array_equal(image, e["own"]["image"]) and np.array_equal(mask, e["own"]["mask"])
            _same(_fill(torch, s, e, image, mask, mask), _want(e, image, mask, mask))
            dense_call(s, e)
            _same(_fill(torch, s, e, image, mask, mask), _want(e, image, mask, mask))


# ---------------------------------------------------------------------------------------------------
# the clip
# ---------------------------------------------------------------------------------------------------
TRIALS = 20


@pytest.fixture(scope="module")
def clip(rsdsfm):
    """tests/test_gpu_stabilize.py's clip"""
    rows, cols, gamma = 96, 128, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, 3.0)
    frames, _, _ = rsdsfm.synth.render_sequence(5, rows, cols, K, v, w, k, gamma, seed=21, speeds=(1.0, 1.4, 0.8, 1.0))
    return frames, rows, cols, K, gamma, [3 + 5 * i for i in range(4)]


def _clip_run(rsdsfm, torch, clip, batch, fused, radius, translation, one_call):
    """the filled clip on a fresh context: rsdsfm_stabilize_video_filled_dev, or rsdsfm_stabilize_video_dev and the loop of public calls"""
    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)]
    d_fused = [torch.full((rows * cols,), np.nan, dtype=torch.float64, device=dev) for _ in range(n)] if fused else None
    d_stab = [torch.full_like(d_frames[0], 77) for _ in range(n)]
    d_smask = [torch.full((rows, cols), 77, dtype=torch.uint8, device=dev) for _ in range(n)]
    d_source = [torch.full((rows, cols), GUARD, dtype=torch.uint8, device=dev) for _ in range(n)]
    dms, Rs, ts = _buffers(torch, dev, n, rows, cols)
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a] if a is not None else None
    sigma = 1.0  # five frames: a window that has neighbours on both sides
    with rsdsfm.Solver(0) as s:
        if batch:
            s.set_flow_batch(batch)
        if one_call:
            r = s.stabilize_video_filled_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs), ptrs(ts), ptrs(d_stab), ptrs(d_smask),
                                             ptrs(d_source), fill_radius=radius, d_fused=ptrs(d_fused), sigma=sigma, translation=translation, seeds=seeds, trials=TRIALS)
            s.synchronize()
        else:
            r = s.stabilize_video_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs), ptrs(ts), ptrs(d_stab), ptrs(d_smask),
                                      d_fused=ptrs(d_fused), sigma=sigma, translation=translation, seeds=seeds, trials=TRIALS)
            s.synchronize()
            r["own_images"], r["own_masks"] = [t.cpu().numpy() for t in d_stab], [t.cpu().numpy() for t in d_smask]
            d_cnt = torch.zeros((n, 2 + 2 * radius), dtype=torch.int64, device=dev)
            d_cnt[:, 1] = torch.from_numpy(r["valid"]).to(dev)
            for p in range(n):
                d_source[p].copy_(d_smask[p])
            torch.cuda.synchronize()
            src = d_fused if fused else dms
            for p in range(n):
                for q, sid, nM, nm in zip(*rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p, radius)):
                    s.stabilize_fill_frame_dev(d_frames[q].data_ptr(), 3, src[q].data_ptr(), Rs[q].data_ptr(), ts[q].data_ptr(), K, rows, cols, nM, nm, int(sid),
                                               d_stab[p].data_ptr(), d_smask[p].data_ptr(), d_source[p].data_ptr(), d_cnt[p, int(sid):].data_ptr())
            s.synchronize()
            r["counts"] = d_cnt.cpu().numpy()
            r["counts"][:, 0] = rows * cols - r["counts"][:, 1:].sum(axis=1)
        r.update(records=[_record(x, dms[i], Rs[i], ts[i]) for i, x in enumerate(r["pairs"])], images=[t.cpu().numpy() for t in d_stab],
                 masks=[t.cpu().numpy() for t in d_smask], sources=[t.cpu().numpy() for t in d_source], fused=[t.cpu().numpy() for t in d_fused] if fused else None)
    return r


@pytest.mark.parametrize("batch,fused,radius,translation", [(1, False, 2, True), (0, False, 2, True), (0, True, 2, True), (0, False, 1, True), (0, False, 2, False)])
def test_filled_clip_equals_its_parts(rsdsfm, clip, batch, fused, radius, translation):
    import torch

    want = _clip_run(rsdsfm, torch, clip, batch, fused, radius, translation, one_call=False)
    got = _clip_run(rsdsfm, torch, clip, batch, fused, radius, translation, one_call=True)
    npix = 96 * 128
    assert got["records"] == want["records"]
    for name in ("scales", "A", "c", "broken", "A_s", "c_s", "M", "m", "valid", "counts"):  # what stabilize_video_dev also writes is that call's
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name
    assert got["counts"].shape == (4, 2 + 2 * radius)
    for p in range(4):
        for k in ("images", "masks", "sources"):
            assert np.array_equal(got[k][p], want[k][p]), (k, p)
        own = want["own_masks"][p] == 1
        assert np.array_equal(got["images"][p][own], want["own_images"][p][own]) and (got["masks"][p][own] == 1).all()  # changed only where the own mask was 0
        assert set(np.unique(got["masks"][p])) <= {0, 1} and np.array_equal(got["sources"][p] == 1, own)
        counts = got["counts"][p]
        assert counts.sum() == npix and counts[0] == (got["masks"][p] == 0).sum() and counts[1] == got["valid"][p] == own.sum()
        assert np.bincount(got["sources"][p].reshape(-1), minlength=2 + 2 * radius).tolist() == counts.tolist()
        assert counts[0] <= npix - own.sum()  # (how many pixels a solved clip fills depends on the solve)
        if fused:
            assert got["fused"][p].tobytes() == want["fused"][p].tobytes(), p
    print("counts", got["counts"].tolist())


def test_the_clip_call_checks_its_own_arguments(rsdsfm, clip):
    import torch

    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.zeros((rows, cols, 2), dtype=torch.float64, device=dev) for _ in range(4)]
    d_stab = [torch.zeros_like(d_frames[0]) for _ in range(4)]
    d_smask = [torch.zeros((rows, cols), dtype=torch.uint8, device=dev) for _ in range(4)]
    dms, Rs, ts = _buffers(torch, dev, 4, rows, cols)
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a] if a is not None else None
    with rsdsfm.Solver(0) as s:
        call = lambda masks=ptrs(d_smask), sources=None, **kw: s.stabilize_video_filled_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs),
                                                                                         ptrs(ts), ptrs(d_stab), masks, sources, trials=TRIALS, **kw)
        with pytest.raises(rsdsfm.RsdsfmError, match="required"):
            call(masks=[0] * 4)
        for bad in (dict(fill_radius=17), dict(fill_radius=-1), dict(sources=ptrs(d_smask)), dict(sources=[m.data_ptr() + 1 for m in d_smask]), dict(sigma=0.0)):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)


def test_evaluate_real_sequence_with_fill(rsdsfm, clip, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, fill=2): what it returned before, every frame as Solver.stabilize_filled gives it, and the files;
    without fill the keys and values of a call made without the new argument"""
    frames, rows, cols, K, gamma, seeds = clip
    ev = rsdsfm.evaluate.evaluate_real_sequence
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, camera=K, gamma=gamma, out_dir=str(tmp_path / "fill"), trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0, fill=2)
        plain = ev(s, frames, camera=K, gamma=gamma, out_dir=str(tmp_path / "plain"), trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
        ps = out["path_smoothed"]
        again = [s.stabilize_filled(frames, [o["depth_map"] for o in out["pairs"]], [o["R"] for o in out["pairs"]], [o["t"] for o in out["pairs"]], K, out["A"], out["c"],
                                    ps["A_s"], ps["c_s"], out["scales"], p, ps["M"][p], ps["m"][p], radius=2) for p in range(4)]
        with pytest.raises(ValueError):
            ev(s, frames, camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, fill=2)
    assert set(out) == set(plain) | {"stab_filled", "stab_sources", "fill_counts"}
    for name in ("scales", "A", "c", "broken", "stab_valid"):
        assert np.array_equal(np.asarray(out[name]), np.asarray(plain[name])), name
    assert out["fill_counts"].shape == (4, 6)
    for p in range(4):
        assert np.array_equal(out["stabilized"][p], plain["stabilized"][p]) and np.array_equal(out["stab_masks"][p], plain["stab_masks"][p])
        img, mask, source, counts = again[p]
        assert np.array_equal(out["stab_filled"][p], img) and np.array_equal(out["stab_sources"][p], source) and out["fill_counts"][p].tolist() == counts.tolist()
        assert np.array_equal(source == 1, plain["stab_masks"][p] == 1) and counts[1] == plain["stab_valid"][p]
        assert np.array_equal(rsdsfm.formats.read_png(str(tmp_path / "fill" / ("stabilized_filled_%d.png" % p))), img)
        assert np.array_equal(rsdsfm.formats.read_png(str(tmp_path / "fill" / ("stabilized_%d.png" % p))), plain["stabilized"][p])
    lines = (tmp_path / "fill" / "fill.csv").read_text().strip().split("\n")
    assert lines[0] == "pair,none,own,prev1,next1,prev2,next2" and len(lines) == 5 and lines[1].split(",")[1:] == [str(x) for x in out["fill_counts"][0]]
    assert not (tmp_path / "plain" / "fill.csv").exists() and not (tmp_path / "plain" / "stabilized_filled_0.png").exists()
    assert sorted(x.name for x in (tmp_path / "plain").iterdir()) == sorted(x.name for x in (tmp_path / "fill").iterdir() if "fill" not in x.name)
