"""GPU: the retimer (include/rsdsfm_retime.h) bit for bit against its definition (tests/retime_spec_numpy.py) in both library builds -- the merge
alone at the shapes where its kernel can go wrong, the frame call on every case of tests/retime_cases.py against the golden fixture the CPU
suite holds to the definition, 20 seeded random tiny frames, the frame call against the public calls made one after another, argument
errors, alternation with the other calls on one context -- and the clip call on two solved clips against the frame calls made one after
another."""
import os

import numpy as np
import pytest

import rectify_dense_spec_numpy as dense
import retime_cases as cases
import retime_spec_numpy as spec
import stabilize_visible_cases as vcases
from test_gpu_stabilize_search import fold_clip, plain_clip

pytestmark = pytest.mark.gpu

GUARD = 0xCD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_retime_v1.npz")
TIMES = lambda nsources: [0, 0.25, 0.5, 1, 1.75, nsources - 1]


def _guarded(torch, dev, a):
    """a's bytes on the device with 16 guard bytes behind them: (the view of a's shape, the guard)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + 16,), GUARD, dtype=torch.uint8, device=dev)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[:a.size].view(*a.shape), buf[a.size:]


def _outputs(torch, dev, image_shape, plane_shape):
    """the three output planes, never preset (every byte GUARD, and 16 guard bytes behind each), and the counters with a guard on either side"""
    planes = [_guarded(torch, dev, np.full(shape, GUARD, dtype=np.uint8)) for shape in (image_shape, plane_shape, plane_shape)]
    return planes, torch.full((7,), -1, dtype=torch.int64, device=dev)


def _collect(planes, cnt, guards, with_source, with_counts):
    for g in [p[1] for p in planes] + list(guards):
        assert (g.cpu().numpy() == GUARD).all()
    c = cnt.cpu().numpy().tolist()
    assert c[0] == -1 and c[6] == -1 and (with_counts or c[1:6] == [-1] * 5)
    (d_img, _), (d_mask, _), (d_src, _) = planes
    source = d_src.cpu().numpy()
    assert with_source or (source == GUARD).all()
    return dict(image=d_img.cpu().numpy(), mask=d_mask.cpu().numpy(), source=source, counts=c[1:6])


def _merge(torch, s, ia, ma, ib, mb, weight, threshold, with_source=True, with_counts=True):
    """one rsdsfm_retime_merge_dev on guarded layers into guarded, never preset outputs"""
    dev = torch.device("cuda", 0)
    layers = [_guarded(torch, dev, x) if x is not None else (None, None) for x in (ia, ma, ib, mb)]
    planes, cnt = _outputs(torch, dev, ia.shape, ma.shape)
    torch.cuda.synchronize()
    ptr = lambda x: None if x is None else x.data_ptr()
    s.retime_merge_dev(ptr(layers[0][0]), ptr(layers[1][0]), ptr(layers[2][0]), ptr(layers[3][0]), 1 if ia.ndim == 2 else 3, ma.shape[0], ma.shape[1], weight,
                       planes[0][0].data_ptr(), planes[1][0].data_ptr(), planes[2][0].data_ptr() if with_source else None, cnt[1:].data_ptr() if with_counts else None,
                       threshold=threshold)
    s.synchronize()
    for (d, _), host in zip(layers, (ia, ma, ib, mb)):  # the layers are only read
        assert host is None or np.array_equal(d.cpu().numpy(), host)
    return _collect(planes, cnt, [l[1] for l in layers if l[1] is not None], with_source, with_counts)


def _same(got, want, name="", source=True, counts=True):
    for k in ("image", "mask") + (("source",) if source else ()):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert not counts or list(got["counts"]) == list(want["counts"]), (name, got["counts"], want["counts"])


# ---------------------------------------------------------------------------------------------------
# the merge
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_merge_equals_the_definition(rsdsfm, arith, channels):
    """every shape (one word, byte tails of 1 and 3, more than one workgroup), masks with all-zero, all-set and mixed words and values other
    than 0 / 1, the four weights and three thresholds, each optional output absent, b absent; guard bytes behind every plane"""
    import torch

    seen = np.zeros(5, dtype=np.int64)
    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in cases.MERGE_SHAPES:
            ia, ma, ib, mb = cases.merge_layers(*shape, channels)
            for w in cases.MERGE_WEIGHTS:
                for thr in cases.MERGE_THRESHOLDS:
                    want = spec.merge(ia, ma, ib, mb, w, thr)
                    _same(_merge(torch, s, ia, ma, ib, mb, w, thr), want, (shape, w, thr))
                    seen += np.array(want["counts"])
            want = spec.merge(ia, ma, ib, mb, 32769, 24)
            for with_source, with_counts in ((False, True), (True, False), (False, False)):
                _same(_merge(torch, s, ia, ma, ib, mb, 32769, 24, with_source, with_counts), want, shape, with_source, with_counts)
            got = _merge(torch, s, ia, ma, None, None, 0, 24)
            _same(got, spec.merge(ia, ma), (shape, "b absent"))
            assert set(np.unique(got["source"]).tolist()) <= {0, 1}
        assert rsdsfm.retime_merge_launches() == 1
    assert (seen > 0).all()


def test_the_host_convenience_of_the_merge(rsdsfm):
    ia, ma, ib, mb = cases.merge_layers(37, 67, 3)
    want = spec.merge(ia, ma, ib, mb, 20000, 24)
    with rsdsfm.Solver(0) as s:
        img, mask, source, counts = s.retime_merge(ia, ma, ib, mb, 20000)
        _same(dict(image=img, mask=mask, source=source, counts=counts.tolist()), want)
        img, mask, source, counts = s.retime_merge(ia, ma)
        _same(dict(image=img, mask=mask, source=source, counts=counts.tolist()), spec.merge(ia, ma))


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
def _sources(torch, dev, case):
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return [tt(x) for x in case["images"]], [tt(z.T) for z in case["depths"]], [tt(np.asarray(R).reshape(-1, 9)) for R in case["Rs"]], [tt(t) for t in case["ts"]]


def _frame(torch, s, case, with_source=True, with_counts=True):
    """one rsdsfm_retime_frame_dev of a case (the context's knob set to the case's) into guarded, never preset outputs"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    d_i, d_dm, d_R, d_t = _sources(torch, dev, case)
    planes, cnt = _outputs(torch, dev, case["images"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    ptrs = lambda a: [x.data_ptr() for x in a]
    s.set_occlusion_search(case["search"])
    s.retime_frame_dev(ptrs(d_i), 1 if case["images"][0].ndim == 2 else 3, ptrs(d_dm), ptrs(d_R), ptrs(d_t), case["K"], rows, cols, case["M"], case["m"], case["weight"],
                       planes[0][0].data_ptr(), planes[1][0].data_ptr(), planes[2][0].data_ptr() if with_source else None, cnt[1:].data_ptr() if with_counts else None,
                       window=case["window"], threshold=case["threshold"], occlusion=case["occlusion"], occlusion_tol_q16=case["tol_q16"], mode=case["mode"],
                       q5_mode=case["q5_mode"], iterations=case["iterations"])
    s.synchronize()
    s.set_occlusion_search(0)
    return _collect(planes, cnt, (), with_source, with_counts)


def _parts(torch, s, case, how):
    """the public calls one after another: every source rendered alone onto zeroed planes by `how` ("window", "visible" or "search"), then
    rsdsfm_retime_merge_dev"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["images"][0].ndim == 2 else 3
    d_i, d_dm, d_R, d_t = _sources(torch, dev, case)
    layers = [(torch.zeros_like(d_i[0]), torch.zeros((rows, cols), dtype=torch.uint8, device=dev)) for _ in d_i]
    planes, cnt = _outputs(torch, dev, case["images"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    kw = dict(mode=case["mode"], q5_mode=case["q5_mode"], iterations=case["iterations"])
    for k, (limg, lmask) in enumerate(layers):
        args = (d_i[k].data_ptr(), ch, d_dm[k].data_ptr(), d_R[k].data_ptr(), d_t[k].data_ptr(), case["K"], rows, cols, case["M"][k], case["m"][k], 1 + k, case["window"],
                limg.data_ptr(), lmask.data_ptr())
        if how == "window":
            s.stabilize_window_frame_dev(*args, **kw)
        else:
            (s.stabilize_search_frame_dev if how == "search" else s.stabilize_visible_frame_dev)(*args, tol_q16=case["tol_q16"], **kw)
    b = layers[1] if len(layers) == 2 else (None, None)
    ptr = lambda x: None if x is None else x.data_ptr()
    s.retime_merge_dev(layers[0][0].data_ptr(), layers[0][1].data_ptr(), ptr(b[0]), ptr(b[1]), ch, rows, cols, case["weight"], planes[0][0].data_ptr(),
                       planes[1][0].data_ptr(), planes[2][0].data_ptr(), cnt[1:].data_ptr(), threshold=case["threshold"])
    s.synchronize()
    return _collect(planes, cnt, (), True, True)


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_every_case_equals_the_definition(oracle, rsdsfm, arith):
    """image, mask, source and the five counts of every fixture case: gray and BGR, one and two sources, a zoom window, the three render calls"""
    import torch

    g = np.load(GOLDEN)
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in cases.all_cases(oracle.pose_table):
            n = case["name"] + "/"
            want = dict(image=g[n + "image"], mask=g[n + "mask"], source=g[n + "source"], counts=g[n + "counts"].tolist())
            _same(_frame(torch, s, case), want, case["name"])
            rows, cols = case["depths"][0].shape
            assert rsdsfm.retime_launches(rows, cols, len(case["images"])) == len(case["images"]) * rsdsfm.stabilize_window_launches(rows, cols) + 1


def test_the_shift_scene_is_exact_on_the_device(rsdsfm):
    """the exact case, derived from the shift alone: bands of SHIFT / 2 columns from one layer each, the rest dissolved to either layer's bytes,
    nothing in conflict"""
    import torch

    case = cases.shift_case()
    rows, cols, half = 24, 40, cases.SHIFT // 2
    with rsdsfm.Solver(0) as s:
        got = _frame(torch, s, case)
        img, mask, source, counts = s.retime(case["images"], case["depths"], case["Rs"], case["ts"], case["K"], case["M"], case["m"], case["weight"])
    assert got["counts"] == [0, half * rows, half * rows, (cols - 2 * half) * rows, 0] == counts.tolist()
    assert np.array_equal(got["image"][:, :cols - half], case["images"][0][:, half:]) and np.array_equal(got["image"][:, half:], case["images"][1][:, :cols - half])
    assert (got["mask"] == 1).all() and (got["source"][:, :half] == 1).all() and (got["source"][:, cols - half:] == 2).all() and (got["source"][:, half:cols - half] == 3).all()
    assert np.array_equal(img, got["image"]) and np.array_equal(mask, got["mask"]) and np.array_equal(source, got["source"])


def test_random_tiny_frames(rsdsfm):
    """20 seeded draws: rows, cols in 2 .. 70, gray or BGR, any weight, four thresholds, the three render calls; every one of the five counts
    occurs (tests/test_retime_cpu.py holds the draws to that on the spec alone)"""
    import torch

    seen = np.zeros(5, dtype=np.int64)
    with rsdsfm.Solver(0) as s:
        for seed in range(20):
            case = cases.random_case(seed)
            want = cases.run_spec(case)
            _same(_frame(torch, s, case), want, case["name"])
            seen += np.array(want["counts"])
    assert (seen > 0).all()


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_the_frame_call_equals_the_public_calls(rsdsfm, arith):
    """occlusion 0, occlusion 1 with the knob at 0 and occlusion 1 with the knob at 1: the public render calls and the public merge one after
    another; and each optional output absent"""
    import torch

    with rsdsfm.Solver(0, arith=arith) as s:
        for occ, knob, how in ((0, 0, "window"), (0, 1, "window"), (1, 0, "visible"), (1, 1, "search")):
            for case in (cases.fold_pair(37, 67, 3, occ, knob), cases.smooth_pair(33, 70, 1, 9, 45000, occlusion=occ, search=knob),
                         cases.one_source(cases.fold_pair(24, 40, 3, occ, knob), "one")):
                want = _parts(torch, s, case, how)
                _same(_frame(torch, s, case), want, (case["name"], how))
                _same(want, cases.run_spec(dict(case, search=knob if occ else 0)), (case["name"], how, "spec"))
        case = cases.fold_pair(37, 67, 3)
        want = cases.run_spec(case)
        for with_source, with_counts in ((False, True), (True, False), (False, False)):
            _same(_frame(torch, s, case, with_source, with_counts), want, "optional", with_source, with_counts)


def test_dense_window_search_and_retime_calls_alternate_on_one_context(oracle, rsdsfm):
    """dense -> window -> search -> retime at one size -> retime at another size -> retime at the first again, on ONE context (one workspace; the
    second layer comes with the first two-source call and again after the size change): each gives its own definition's bytes"""
    import torch

    import stabilize_search_cases as scases
    from test_gpu_stabilize_search import _render
    from test_gpu_stabilize_search import _same as _same3

    dev = torch.device("cuda", 0)
    a = scases.fold_case(37, 67, 3, 1, mask0=scases.pattern_mask(37, 67))
    one, two, other = cases.one_source(cases.fold_pair(37, 67, 3), "one"), cases.fold_pair(37, 67, 3, 1, 1), cases.smooth_pair(33, 70, 1, 9, 45000)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    with rsdsfm.Solver(0) as s:
        d_img, d_dm, d_R, d_t = tt(a["image"]), tt(a["depth"].T), tt(a["R"]), tt(a["t"])
        out, d_mask = torch.full_like(d_img, 77), torch.full((37, 67), 77, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        s.rectify_dense_frame_dev(d_img.data_ptr(), 3, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), a["K"], 37, 67, out.data_ptr(), d_mask.data_ptr())
        s.synchronize()
        want = dense.rectify_dense(a["image"], a["depth"], a["R"], a["t"], *a["K"])
        assert np.array_equal(out.cpu().numpy(), want["image"]) and np.array_equal(d_mask.cpu().numpy(), want["mask"])
        _same3(_render(torch, s, a, "window"), dict(vcases.run_spec(a, visible=False), counts=vcases.run_spec(a, visible=False)["counts"][:1]))
        _same3(_render(torch, s, a), scases.run_spec(a))
        _same(_frame(torch, s, one), cases.run_spec(one), "one source first: no second layer yet")
        _same(_frame(torch, s, two), cases.run_spec(two), "two sources")
        _same(_frame(torch, s, other), cases.run_spec(other), "another size")
        _same3(_render(torch, s, a), scases.run_spec(a))
        _same(_frame(torch, s, two), cases.run_spec(two), "the first size again")


def test_argument_errors(rsdsfm):
    """after each refused call the same call without the fault goes through"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)
    ia, ib, out = u8(rows, cols, 3), u8(rows, cols, 3), u8(rows, cols + 4, 3)
    ma, mb, mask, source = u8(rows, cols), u8(rows, cols), u8(rows, cols + 4), u8(rows, cols + 4)
    counts = torch.full((7,), -1, dtype=torch.int64, device=dev)
    dm, t = torch.ones(rows * cols, dtype=torch.float64, device=dev), torch.zeros(rows * 3, dtype=torch.float64, device=dev)
    R = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 9).repeat(rows, 1).contiguous()
    K = (50.0, 50.0, 32.0, 8.0)
    M2, m2 = np.stack([np.eye(3)] * 2), np.zeros((2, 3))
    nanM = M2.copy()
    nanM[1, 1, 2] = np.nan
    infm = m2.copy()
    infm[0, 1] = np.inf
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        merge = lambda a=ia.data_ptr(), ka=ma.data_ptr(), b=ib.data_ptr(), kb=mb.data_ptr(), ch=3, r=rows, c=cols, w=100, o=out.data_ptr(), k=mask.data_ptr(), **kw: \
            s.retime_merge_dev(a, ka, b, kb, ch, r, c, w, o, k, **kw)
        for bad in (dict(a=0), dict(ka=0), dict(o=0), dict(k=0), dict(b=0), dict(kb=0), dict(b=None, kb=None), dict(a=ia.data_ptr() + 1), dict(kb=mb.data_ptr() + 2),
                    dict(o=out.data_ptr() + 1), dict(d_source=source.data_ptr() + 3), dict(o=ia.data_ptr()), dict(k=mb.data_ptr()), dict(d_source=ma.data_ptr()),
                    dict(d_source=mask.data_ptr()), dict(k=out.data_ptr()), dict(ch=2), dict(ch=4), dict(w=-1), dict(w=65536), dict(threshold=256), dict(threshold=-1),
                    dict(d_counts5=counts.data_ptr() + 4), dict(r=1), dict(c=16385)):
            with pytest.raises(rsdsfm.RsdsfmError):
                merge(**bad)
            merge()  # the same call without the fault goes through
        merge(b=None, kb=None, w=0, d_source=source.data_ptr(), d_counts5=counts[1:].data_ptr(), threshold=0)
        s.synchronize()
        assert counts.cpu().numpy().tolist() == [-1, rows * cols, 0, 0, 0, 0, -1]  # both masks empty

        src = lambda n: ([ia.data_ptr(), ib.data_ptr()][:n], [dm.data_ptr()] * n, [R.data_ptr()] * n, [t.data_ptr()] * n)
        bad_bytes = rsdsfm.RetimeParams()
        bad_bytes.threshold, bad_bytes.struct_bytes = 24, 16

        def frame(n=2, M=M2, m=m2, w=100, o=out.data_ptr(), k=mask.data_ptr(), ch=3, r=rows, c=cols, images=None, **kw):
            i, d, rr, tt = src(min(max(n, 1), 2))
            i = images if images is not None else i
            if n not in (1, 2):  # the wrapper counts its list: nsrc = 0 or 3 through lists of that length
                i, d, rr, tt = ([x[0]] * n for x in (i, d, rr, tt))
            s.retime_frame_dev(i, ch, d, rr, tt, K, r, c, M, m, w, o, k, **kw)

        for bad in (dict(n=0), dict(n=3), dict(n=1), dict(w=-1), dict(w=65536), dict(M=nanM), dict(m=infm), dict(M=None), dict(threshold=256), dict(threshold=-1),
                    dict(occlusion=2), dict(occlusion_tol_q16=65537), dict(occlusion_tol_q16=-1), dict(params=bad_bytes), dict(o=0), dict(k=0), dict(o=out.data_ptr() + 2),
                    dict(d_source=mask.data_ptr()), dict(o=ia.data_ptr()), dict(d_counts5=counts.data_ptr() + 4), dict(images=[ia.data_ptr(), 0]), dict(ch=2),
                    dict(window=(0, 0, 0, 8)), dict(window=(9, 0, 8, 32)), dict(iterations=17), dict(mode=2), dict(r=1)):
            with pytest.raises(rsdsfm.RsdsfmError):
                frame(**bad)
            frame()  # the same call without the fault goes through
        frame(n=1, w=0)
        frame(M=nanM, n=1, w=0)  # the second pose (the one with the NaN) is not read with one source
        ok_zero = rsdsfm.RetimeParams()  # a zero-initialised struct: threshold 0, no occlusion
        frame(params=ok_zero, d_source=source.data_ptr(), d_counts5=counts[1:].data_ptr())
        s.synchronize()
        assert counts.cpu().numpy().tolist() == [-1, 0, 0, 0, rows * cols, 0, -1]  # constant depth, identity poses, equal (zero) frames: all dissolved
        with pytest.raises(rsdsfm.RsdsfmError):  # the clip call: a time outside the path is refused before anything is enqueued
            s.retime_video_dev([ia.data_ptr(), ib.data_ptr()], rows, cols, 3, K, [dm.data_ptr()] * 2, [R.data_ptr()] * 2, [t.data_ptr()] * 2, M2, m2, M2, m2, np.ones(2),
                               [0.5, 1.5], [out.data_ptr()] * 2, [mask.data_ptr()] * 2)
        r = s.retime_video_dev([ia.data_ptr(), ib.data_ptr()], rows, cols, 3, K, [dm.data_ptr()] * 2, [R.data_ptr()] * 2, [t.data_ptr()] * 2, M2, m2, M2, m2, np.ones(2),
                               [0.5, 1.0], [out.data_ptr()] * 2, [mask.data_ptr()] * 2)
        assert r["sources"].tolist() == [[0, 1], [1, -1]] and r["weights"].tolist() == [32768, 0] and r["counts"].sum(axis=1).tolist() == [rows * cols] * 2


# ---------------------------------------------------------------------------------------------------
# the clip call
# ---------------------------------------------------------------------------------------------------
TRIALS = 20


@pytest.mark.parametrize("last_frame", [False, True])
@pytest.mark.parametrize("which", ["plain-16x64", "fold-24x40"])
def test_the_clip_call_equals_the_frame_calls(rsdsfm, which, last_frame):
    """on the two solved clips of tests/test_gpu_stabilize_search.py, after rsdsfm_stabilize_video_dev (with and without last_frame): every plane
    and host array of rsdsfm_retime_video_dev at times [0, 0.25, 0.5, 1, 1.75, nsources - 1] is byte for byte rsdsfm_retime_poses and
    rsdsfm_retime_frame_dev made one after another, and at integer times image and mask are the own frame's rsdsfm_stabilize_window_frame_dev
    render through the full window.  The plain clip without last_frame has two sources, so 1.75 lies outside its path: there the whole list
    is seen to be refused, and the run is made with the times inside [0, nsources - 1]"""
    import torch

    frames, rows, cols, K, gamma, seeds, _ = (plain_clip if which.startswith("plain") else fold_clip)(rsdsfm)
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    ns = n + (1 if last_frame else 0)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.zeros((rows, cols, 2), dtype=torch.float64, device=dev) for _ in range(n)]
    plane = lambda value, count: [torch.full((rows, cols), value, dtype=torch.uint8, device=dev) for _ in range(count)]
    image = lambda value, count: [torch.full_like(d_frames[0], value) for _ in range(count)]
    d_stab, d_smask = image(77, ns), plane(77, ns)
    dms = [torch.zeros(rows * cols, dtype=torch.float64, device=dev) for _ in range(ns)]
    Rs = [torch.zeros((rows, 9), dtype=torch.float64, device=dev) for _ in range(ns)]
    ts = [torch.zeros((rows, 3), dtype=torch.float64, device=dev) for _ in range(ns)]
    times = TIMES(ns)
    inside = [t for t in times if t <= ns - 1]
    assert len(inside) == len(times) or (which.startswith("plain") and not last_frame and inside == [0, 0.25, 0.5, 1, 1])
    nt = len(inside)
    d_out, d_omask, d_osrc = image(GUARD, nt), plane(GUARD, nt), plane(GUARD, nt)
    d_one, d_onemask, d_onesrc = image(55, nt), plane(55, nt), plane(55, nt)
    d_cnt = torch.zeros((nt, 5), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ptrs = lambda a: [x.data_ptr() for x in a]
    with rsdsfm.Solver(0) as s:
        r = s.stabilize_video_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs), ptrs(ts), ptrs(d_stab), ptrs(d_smask), sigma=1.0, seeds=seeds,
                                  trials=TRIALS, last_frame=last_frame)
        s.synchronize()
        assert len(r["scales"]) == ns
        clip = (ptrs(d_frames), rows, cols, 3, K, ptrs(dms), ptrs(Rs), ptrs(ts), r["A"], r["c"], r["A_s"], r["c_s"], r["scales"])
        if len(inside) < len(times):
            with pytest.raises(rsdsfm.RsdsfmError):
                s.retime_video_dev(*clip, times, ptrs(d_out) + [d_out[0].data_ptr()], ptrs(d_omask) + [d_omask[0].data_ptr()])
            s.synchronize()
            assert all((x.cpu().numpy() == GUARD).all() for x in d_out + d_omask)  # nothing was enqueued
        got = s.retime_video_dev(*clip, inside, ptrs(d_out), ptrs(d_omask), ptrs(d_osrc))
        s.synchronize()
        want_sources, want_weights = [], []
        for i, t in enumerate(inside):
            src, w, M, m, _, _ = rsdsfm.retime_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], t, nsources=ns)
            s.retime_frame_dev([d_frames[q].data_ptr() for q in src], 3, [dms[q].data_ptr() for q in src], [Rs[q].data_ptr() for q in src],
                               [ts[q].data_ptr() for q in src], K, rows, cols, M, m, w, d_one[i].data_ptr(), d_onemask[i].data_ptr(), d_onesrc[i].data_ptr(),
                               d_cnt[i].data_ptr())
            want_sources.append(list(src) + [-1] * (2 - len(src)))
            want_weights.append(w)
        s.synchronize()
        assert got["sources"].tolist() == want_sources and got["weights"].tolist() == want_weights
        assert got["counts"].tobytes() == d_cnt.cpu().numpy().tobytes() and (got["counts"].sum(axis=1) == rows * cols).all()
        for i in range(nt):
            for a, b in ((d_out, d_one), (d_omask, d_onemask), (d_osrc, d_onesrc)):
                assert np.array_equal(a[i].cpu().numpy(), b[i].cpu().numpy()), (i, inside[i])
            bins = np.bincount(d_osrc[i].cpu().numpy().reshape(-1), minlength=6)
            assert [bins[0], bins[1], bins[2], bins[3], bins[4] + bins[5]] == got["counts"][i].tolist()
        print(which, "last_frame", last_frame, "times", inside, "counts", got["counts"].tolist())
        # integer times: the own frame's window render through the full window, onto zeroed planes
        d_own, d_ownmask = torch.zeros_like(d_frames[0]), torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
        for i, t in enumerate(inside):
            if t != int(t):
                continue
            q = int(t)
            d_own.zero_()
            d_ownmask.zero_()
            torch.cuda.synchronize()
            s.stabilize_window_frame_dev(d_frames[q].data_ptr(), 3, dms[q].data_ptr(), Rs[q].data_ptr(), ts[q].data_ptr(), K, rows, cols, r["M"][q], r["m"][q], 1,
                                         (0, 0, rows, cols), d_own.data_ptr(), d_ownmask.data_ptr())
            s.synchronize()
            assert np.array_equal(d_out[i].cpu().numpy(), d_own.cpu().numpy()) and np.array_equal(d_omask[i].cpu().numpy(), d_ownmask.cpu().numpy()), t
            assert got["weights"][i] == 0 and got["sources"][i].tolist() == [q, -1]
        # without the counts the call only enqueues: the same planes
        again = s.retime_video_dev(*clip, inside, ptrs(d_one), ptrs(d_onemask), want_counts=False)
        s.synchronize()
        assert "counts" not in again and again["sources"].tolist() == want_sources
        for i in range(nt):
            assert np.array_equal(d_out[i].cpu().numpy(), d_one[i].cpu().numpy())


def test_evaluate_real_sequence_with_retime(rsdsfm, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, retime=2) adds exactly retimed, retime_masks, retime_sources, retime_counts, retime_times and
    the files retimed_<i>.png and retime.csv; without the keyword every key and file is what it was"""
    frames, rows, cols, K, gamma, seeds, _ = plain_clip(rsdsfm)
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
    n = len(frames) - 1
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, retime=2, out_dir=str(tmp_path / "with"), **kw)
        plain = ev(s, frames, out_dir=str(tmp_path / "without"), **kw)
        listed = ev(s, frames, retime=[0.5], **kw)
        ps = out["path_smoothed"]
        src, w, M, m, _, _ = rsdsfm.retime_poses(out["A"], out["c"], ps["A_s"], ps["c_s"], out["scales"], 0.5, nsources=n)
        o = out["pairs"]
        img, mask, source, counts = s.retime([frames[q] for q in src], [o[q]["depth_map"] for q in src], [o[q]["R"] for q in src], [o[q]["t"] for q in src], K, M, m, w)
    assert set(out) == set(plain) | {"retimed", "retime_masks", "retime_sources", "retime_counts", "retime_times"}
    assert out["retime_times"].tolist() == rsdsfm.retime_times(n, 2).tolist() == [i / 2 for i in range(2 * (n - 1) + 1)]
    nt = len(out["retime_times"])
    assert len(out["retimed"]) == len(out["retime_masks"]) == len(out["retime_sources"]) == nt and out["retime_counts"].shape == (nt, 5)
    assert np.array_equal(out["retimed"][1], img) and np.array_equal(out["retime_masks"][1], mask) and np.array_equal(out["retime_sources"][1], source)
    assert out["retime_counts"][1].tolist() == counts.tolist() and np.array_equal(listed["retimed"][0], img)
    for i in range(nt):
        assert out["retimed"][i].shape == frames[0].shape and out["retime_counts"][i].sum() == rows * cols
    for k in plain:
        if k not in ("pairs", "path_smoothed", "links"):
            assert np.asarray(out[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    with_files, without_files = set(os.listdir(str(tmp_path / "with"))), set(os.listdir(str(tmp_path / "without")))
    assert with_files == without_files | {"retimed_%d.png" % i for i in range(nt)} | {"retime.csv"}
    lines = open(str(tmp_path / "with" / "retime.csv")).read().split()
    assert lines[0] == "index,time,source_a,source_b,weight_q16,none,a_only,b_only,dissolved,conflict" and len(lines) == 1 + nt
    assert lines[2] == ",".join(["1", "0.5", "0", "1", "32768"] + [str(int(x)) for x in out["retime_counts"][1]])
