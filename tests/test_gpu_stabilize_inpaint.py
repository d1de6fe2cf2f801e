"""GPU: the inpainting (include/rsdsfm_stabilize_inpaint.h) bit for bit against its definition (tests/stabilize_inpaint_spec_numpy.py) in both
library builds, with guard bytes behind every plane -- sizes whose rows do not start on a dword, sizes that are odd at every level, one row of
cells, and the smallest frame with a large pull, the single-workgroup launch and two large pushes; 1 and 3 channels; with and without the
source plane and the counter; the argument errors; one context shared with the dense, stabilise, fill, crop and blend calls -- the clip call
(rsdsfm_stabilize_video_inpainted_dev) byte for byte against the public calls made one after another, and evaluate_real_sequence(inpaint=True).
The clip is tests/test_gpu_stabilize.py's, built by tests/test_gpu_stabilize_blend.py's fixture."""
import numpy as np
import pytest

import stabilize_blend_spec_numpy as blend_spec
import stabilize_cases as stab_cases
import stabilize_inpaint_cases as cases
import stabilize_inpaint_spec_numpy as spec
from test_gpu_stabilize_blend import GUARD, M_N, TRIALS, _blend, _blend_want, _clean, _distance, _guarded, _pair, _same, _window_call, clip, m_N  # noqa: F401

pytestmark = pytest.mark.gpu


def _frame(torch, s, image, mask, with_source=True, with_count=True):
    """rsdsfm_inpaint_frame_dev on guarded planes; the counter has a guard word on either side.  -> (image, source, count)"""
    dev = torch.device("cuda", 0)
    rows, cols = mask.shape
    (d_img, g0), (d_mask, g1), (d_src, g2) = _guarded(torch, dev, image), _guarded(torch, dev, mask), _guarded(torch, dev, np.zeros_like(mask))
    cnt = torch.full((3,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s.inpaint_frame_dev(d_img.data_ptr(), d_mask.data_ptr(), 1 if image.ndim == 2 else 3, rows, cols, d_src.data_ptr() if with_source else None,
                        cnt[1:].data_ptr() if with_count else None)
    s.synchronize()
    _clean(g0, g1, g2)
    assert np.array_equal(d_mask.cpu().numpy(), mask)  # only read
    c = cnt.cpu().numpy()
    assert c[0] == -7 and c[2] == -7 and (with_count or c[1] == -7)
    src = d_src.cpu().numpy()
    assert with_source or not src.any()
    return d_img.cpu().numpy(), src, int(c[1])


_expected = {}


def _case(shape, ch, name, mask):
    """the image and the spec's (image, source, count), computed once and shared by both builds"""
    key = (shape, ch, name)
    if key not in _expected:
        image = cases.image_of(shape[0], shape[1], ch, 13 * shape[0] + shape[1] + ch)
        out, source = image.copy(), np.zeros(shape, dtype=np.uint8)
        _expected[key] = (image, out, source, spec.inpaint(out, mask, source))
    return _expected[key]


def _masks(shape):
    rows, cols = shape
    return cases.masks(rows, cols, rows + 3 * cols) + ([("hole", cases.big_hole(rows, cols, 5))] if shape == (401, 603) else [])


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_frame_equals_the_spec(rsdsfm, arith):
    import torch

    assert rsdsfm.inpaint_launches(401, 603) == 6  # level 0 -> 1, ONE large pull, the single-workgroup launch, TWO large pushes, the output
    assert all(rsdsfm.inpaint_launches(*shape) == 3 for shape in cases.GPU_SIZES[:-1])  # nothing smaller in the list has a large level
    written = 0
    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in cases.GPU_SIZES:
            for ch in (1, 3):
                for name, mask in _masks(shape):
                    image, want_image, want_source, want_count = _case(shape, ch, name, mask)
                    got = _frame(torch, s, image, mask)
                    assert np.array_equal(got[0], want_image) and np.array_equal(got[1], want_source) and got[2] == want_count, (shape, ch, name)
                    if name in ("set", "empty"):
                        assert got[2] == 0 and np.array_equal(got[0], image) and not got[1].any()
                    written += got[2]
                name, mask = _masks(shape)[3]  # the bands: without the source plane, without the counter, without either
                image, want_image, want_source, want_count = _case(shape, ch, name, mask)
                for with_source, with_count in ((False, True), (True, False), (False, False)):
                    got = _frame(torch, s, image, mask, with_source, with_count)
                    assert np.array_equal(got[0], want_image) and (not with_source or np.array_equal(got[1], want_source)), (shape, ch, with_source, with_count)
                    assert not with_count or got[2] == want_count
        image, mask = cases.image_of(33, 70, 3, 1), cases.masks(33, 70, 2)[3][1]
        out, source, count = s.inpaint(image, mask)  # the host convenience
        want, want_source = image.copy(), np.zeros_like(mask)
        assert count == spec.inpaint(want, mask, want_source) and np.array_equal(out, want) and np.array_equal(source, want_source)
    assert written > 500000
    m = cases.big_hole(401, 603, 5)
    assert not m[133:283:8, 150:350:8].any() and not spec.pyramid(np.zeros((401, 603), dtype=np.uint8), m)[1][4].all()  # cells stay invalid 4 levels up


def test_argument_errors(rsdsfm):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    plane = lambda ch=1: torch.zeros(rows * cols * ch + 8, dtype=torch.uint8, device=dev)
    image, mask, source = plane(3), plane(), plane()
    cnt = torch.zeros(3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    P = lambda t: t.data_ptr()
    with rsdsfm.Solver(0) as s:
        ok = dict(i=P(image), m=P(mask), ch=3, r=rows, c=cols, s=P(source), cnt=P(cnt))
        for bad in (dict(i=0), dict(m=0), dict(i=P(image) + 1), dict(m=P(mask) + 2), dict(s=P(source) + 3), dict(cnt=P(cnt) + 4), dict(ch=2), dict(ch=0), dict(ch=4),
                    dict(r=1), dict(c=1), dict(r=16385), dict(c=16385), dict(s=P(mask)), dict(s=P(image)), dict(i=P(mask))):
            a = dict(ok, **bad)
            with pytest.raises(rsdsfm.RsdsfmError):
                s.inpaint_frame_dev(a["i"], a["m"], a["ch"], a["r"], a["c"], a["s"], a["cnt"])
        s.inpaint_frame_dev(ok["i"], ok["m"], 3, rows, cols, ok["s"], ok["cnt"])  # the same arguments without a fault go through
        s.inpaint_frame_dev(ok["i"], ok["m"], 1, rows, cols, None, None)
        s.synchronize()
    assert not image.any() and not source.any() and cnt.cpu().numpy().tolist() == [0, 0, 0]  # an empty mask changes nothing


def test_inpaint_dense_stabilise_fill_crop_and_blend_alternate_on_one_context(oracle, rsdsfm):
    """inpaint, distance, blend, dense, stabilise, fill, window-search and window-frame calls at two sizes on ONE context (one workspace,
    rebuilt only when the size changes, the pyramid of cells with it): the spec's result every time, the inpainting's before and after the
    others have used the workspace"""
    import torch

    import stabilize_crop_spec_numpy as crop_spec

    dev = torch.device("cuda", 0)
    a, b = _pair(oracle, (33, 70), 3), _pair(oracle, (96, 128), 1)
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    def inpainted(s, image, mask, some=False):
        want, want_source = image.copy(), np.zeros_like(mask)
        want_count = spec.inpaint(want, mask, want_source)
        got = _frame(torch, s, image, mask)
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want_source) and got[2] == want_count and (want_count > 0 or not some)

    with rsdsfm.Solver(0) as s:
        for e in (a, b, a):
            rows, cols = e["depth"].shape
            ch = 1 if e["image"].ndim == 2 else 3
            image, mask = e["own"]["image"], e["own"]["mask"]
            inpainted(s, image, mask, some=True)  # first on the new size: the workspace and the pyramid are made here
            assert np.array_equal(_distance(torch, s, mask, 16), blend_spec.seam_distance(mask, 16))
            d_img, d_dm, d_R, d_t = tt(e["image"]), tt(e["depth"].T), tt(e["R"]), tt(e["t"])
            out, d_mask = torch.full_like(d_img, 77), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            s.rectify_dense_frame_dev(d_img.data_ptr(), ch, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, out.data_ptr(), d_mask.data_ptr())
            s.synchronize()
            dense, dense_mask = out.cpu().numpy(), d_mask.cpu().numpy()
            inpainted(s, dense, dense_mask)  # the generic call on the dense rectifier's output
            s.stabilize_frame_dev(d_img.data_ptr(), ch, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, stab_cases.M_STD, stab_cases.m_STD,
                                  out.data_ptr(), d_mask.data_ptr())
            s.synchronize()
            assert np.array_equal(out.cpu().numpy(), image) and np.array_equal(d_mask.cpu().numpy(), mask)
            window = s.crop_window_dev([d_mask.data_ptr()], rows, cols, rows * cols // 50, 0)
            assert window == crop_spec.crop_window(mask[None], max_empty=rows * cols // 50, margin=0)
            layer = _window_call(torch, s, e, np.zeros_like(image), np.zeros_like(mask), np.zeros_like(mask), window, with_source=False)
            case = dict(image=image, mask=mask, source=mask, dist=_distance(torch, s, mask, 8), layer=layer["image"], lmask=layer["mask"])
            blended = _blend(torch, s, case, 8, min_overlap=64)
            _same(blended, _blend_want(case, 8, min_overlap=64))
            inpainted(s, blended["image"], blended["mask"])
            d_fill, d_fmask, d_n, d_ndm = tt(image), tt(mask), tt(e["nimage"]), tt(e["ndepth"].T)
            torch.cuda.synchronize()
            s.stabilize_fill_frame_dev(d_n.data_ptr(), ch, d_ndm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, M_N, m_N, 2,
                                       d_fill.data_ptr(), d_fmask.data_ptr())
            s.synchronize()
            full = _window_call(torch, s, e, image, mask, mask, (0, 0, rows, cols))
            assert np.array_equal(d_fill.cpu().numpy(), full["image"]) and np.array_equal(d_fmask.cpu().numpy(), full["mask"])
            inpainted(s, full["image"], full["mask"])


# ---------------------------------------------------------------------------------------------------
# the clip
# ---------------------------------------------------------------------------------------------------
def _clip_run(rsdsfm, torch, clip, channels, radius, window_in, host_arrays, one_call, with_sources=True, margin=0, max_empty=200, inpaint_ptrs=None):
    """the inpainted clip on a fresh context: rsdsfm_stabilize_video_inpainted_dev, or the blended clip call and the loop of public calls"""
    frames, rows, cols, K, gamma, seeds = clip
    if channels == 1:
        frames = np.ascontiguousarray(frames[..., 1])
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)]
    planes = lambda value, like=None: [torch.full_like(d_frames[0], value) if like else torch.full((rows, cols), value, dtype=torch.uint8, device=dev) for _ in range(n)]
    d_stab, d_smask, d_source = planes(77, True), planes(77), planes(GUARD)
    d_crop, d_cmask, d_csource = planes(55, True), planes(55), planes(55)
    d_blend, d_bmask, d_bsource = planes(33, True), planes(33), planes(33)
    inp = [_guarded(torch, dev, np.full(frames[0].shape, 11, dtype=np.uint8)) for _ in range(n)]
    isrc = [_guarded(torch, dev, np.full((rows, cols), 11, dtype=np.uint8)) for _ in range(n)]
    d_inp, d_isrc = [t for t, _ in inp], [t for t, _ in isrc]
    dms = [torch.zeros(rows * cols, dtype=torch.float64, device=dev) for _ in range(n)]
    Rs = [torch.zeros((rows, 9), dtype=torch.float64, device=dev) for _ in range(n)]
    ts = [torch.zeros((rows, 3), dtype=torch.float64, device=dev) for _ in range(n)]
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a]
    common = dict(window_in=window_in, max_empty=max_empty, margin=margin, d_sources=ptrs(d_source), fill_radius=radius, sigma=1.0, seeds=seeds, trials=TRIALS,
                  blend_feather=8, blend_min_overlap=64, want_gains=host_arrays, want_blend_counts=host_arrays, d_crop_sources=ptrs(d_csource))
    head = (ptrs(d_frames), rows, cols, channels, K, gamma, ptrs(dms), ptrs(d_flows), ptrs(Rs), ptrs(ts), ptrs(d_stab), ptrs(d_smask), ptrs(d_crop), ptrs(d_cmask),
            ptrs(d_blend), ptrs(d_bmask), ptrs(d_bsource))
    with rsdsfm.Solver(0) as s:
        if one_call:
            ip, sp = inpaint_ptrs(ptrs(d_inp), ptrs(d_isrc), ptrs(d_blend), ptrs(d_bmask), ptrs(d_bsource)) if inpaint_ptrs else (ptrs(d_inp), ptrs(d_isrc))
            r = s.stabilize_video_inpainted_dev(*head, ip, sp if with_sources else None, want_inpaint_counts=host_arrays, **common)
            s.synchronize()
        else:
            r = s.stabilize_video_blended_dev(*head, **common)
            s.synchronize()
            d_cnt = torch.full((n,), -1, dtype=torch.int64, device=dev)
            for p in range(n):
                d_inp[p].copy_(d_blend[p])
                if with_sources:
                    d_isrc[p].copy_(d_bsource[p])
            torch.cuda.synchronize()
            for p in range(n):
                s.inpaint_frame_dev(d_inp[p].data_ptr(), d_bmask[p].data_ptr(), channels, rows, cols, d_isrc[p].data_ptr() if with_sources else None, d_cnt[p:].data_ptr())
            s.synchronize()
            r["inpaint_counts"] = d_cnt.cpu().numpy()
        _clean(*[g for _, g in inp + isrc])
        host = lambda a: [t.cpu().numpy() for t in a]
        r.update(images=host(d_stab), crops=host(d_crop), crop_masks=host(d_cmask), crop_sources=host(d_csource), blends=host(d_blend), blend_masks=host(d_bmask),
                 blend_sources=host(d_bsource), inpainted=host(d_inp), inpaint_sources=host(d_isrc))
    return r


@pytest.mark.parametrize("channels,radius,window_in,host_arrays", [(3, 2, None, True), (1, 0, (7, 11, 60, 80), False)])
def test_inpainted_clip_equals_its_parts(rsdsfm, clip, channels, radius, window_in, host_arrays):
    import torch

    want = _clip_run(rsdsfm, torch, clip, channels, radius, window_in, host_arrays, one_call=False, with_sources=host_arrays)
    got = _clip_run(rsdsfm, torch, clip, channels, radius, window_in, host_arrays, one_call=True, with_sources=host_arrays)
    assert got["window"] == want["window"] and got["window"][2] >= 1
    for name in ("scales", "A", "c", "A_s", "c_s", "M", "m", "valid", "counts", "crop_counts") + (("gains", "blend_counts", "inpaint_counts") if host_arrays else ()):
        assert np.asarray(got[name]).tobytes() == np.asarray(want[name]).tobytes(), name
    assert ("inpaint_counts" in got) == host_arrays
    for p in range(4):
        for k in ("images", "crops", "crop_masks", "crop_sources", "blends", "blend_masks", "blend_sources", "inpainted", "inpaint_sources"):
            assert np.array_equal(got[k][p], want[k][p]), (k, p)  # the blended outputs are the blended call's alone
        seen = got["blend_masks"][p] != 0
        assert seen.any() and np.array_equal(got["inpainted"][p][seen], got["blends"][p][seen])
        if host_arrays:
            assert got["inpaint_counts"][p] == (~seen).sum() == (got["inpaint_sources"][p] == rsdsfm.INPAINT_SOURCE).sum()
            assert np.array_equal(got["inpaint_sources"][p][seen], got["blend_sources"][p][seen]) and got["inpaint_sources"][p].all()
        else:
            assert (got["inpaint_sources"][p] == 11).all()  # not passed: not touched
    if host_arrays:
        print("window", got["window"], "inpaint counts", got["inpaint_counts"].tolist())
        assert got["inpaint_counts"].sum() > 0  # something was invented


def test_a_clip_without_a_window_and_argument_errors(rsdsfm, clip):
    """margin 64 and no empty pixel allowed: nothing fits a solved clip's masks; the blend planes are zero, so the inpaint planes are and the
    counts are 0.  The clip call's own argument errors: a missing, misaligned or aliased inpaint plane."""
    import torch

    want = _clip_run(rsdsfm, torch, clip, 3, 1, None, True, one_call=False, margin=64, max_empty=0)
    got = _clip_run(rsdsfm, torch, clip, 3, 1, None, True, one_call=True, margin=64, max_empty=0)
    assert got["window"] == want["window"] and got["inpaint_counts"].tolist() == want["inpaint_counts"].tolist()
    for k in ("blends", "blend_masks", "blend_sources", "inpainted", "inpaint_sources"):
        assert all(np.array_equal(x, y) for x, y in zip(got[k], want[k])), k
    if got["window"] == (0, 0, 0, 0):  # (what a solved clip's masks hold depends on the solve)
        assert got["inpaint_counts"].tolist() == [0] * 4
        assert not any(x.any() for k in ("blends", "blend_masks", "inpainted", "inpaint_sources") for x in got[k])
    swap = lambda i, v: (lambda a: a[:i] + [v(a[i])] + a[i + 1:])
    for bad in (lambda ip, sp, b, bm, bs: (swap(1, lambda x: 0)(ip), sp), lambda ip, sp, b, bm, bs: (ip, swap(2, lambda x: 0)(sp)),
                lambda ip, sp, b, bm, bs: (swap(0, lambda x: x + 1)(ip), sp), lambda ip, sp, b, bm, bs: (ip, swap(3, lambda x: x + 2)(sp)),
                lambda ip, sp, b, bm, bs: (swap(1, lambda x: b[1])(ip), sp), lambda ip, sp, b, bm, bs: (swap(1, lambda x: bm[1])(ip), sp),
                lambda ip, sp, b, bm, bs: (ip, swap(1, lambda x: bm[1])(sp)), lambda ip, sp, b, bm, bs: (ip, swap(1, lambda x: bs[1])(sp)),
                lambda ip, sp, b, bm, bs: (ip, swap(2, lambda x: ip[2])(sp)), lambda ip, sp, b, bm, bs: (None, sp)):
        with pytest.raises(rsdsfm.RsdsfmError):
            _clip_run(rsdsfm, torch, clip, 3, 1, None, True, one_call=True, inpaint_ptrs=bad)
    for kw in (dict(radius=17, window_in=None), dict(radius=1, window_in=(0, 0, 97, 128))):  # the inner call's errors come through
        with pytest.raises(rsdsfm.RsdsfmError):
            _clip_run(rsdsfm, torch, clip, 3, kw["radius"], kw["window_in"], True, one_call=True)


def test_evaluate_real_sequence_with_inpaint(rsdsfm, clip, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, fill=2, crop=True, blend=True, inpaint=True) and with stabilize=True alone: what it
    returned before, frames without a pixel that nobody gave, the files; its ValueError"""
    frames, rows, cols, K, gamma, seeds = clip
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=TRIALS, seeds=seeds, stabilize=True, smooth_sigma=1.0)
    full = dict(fill=2, crop=True, crop_margin=0, crop_max_empty=200, blend=True, blend_feather=8)
    new = {"stab_inpainted", "inpaint_sources", "inpaint_counts"}
    with rsdsfm.Solver(0) as s:
        runs = []
        for name, extra, last, last_mask in (("full", full, "stab_blended", None), ("alone", {}, "stabilized", "stab_masks")):
            out = ev(s, frames, out_dir=str(tmp_path / name), inpaint=True, **dict(kw, **extra))
            plain = ev(s, frames, out_dir=str(tmp_path / (name + "_plain")), **dict(kw, **extra))
            runs.append((name, out, plain, last, last_mask))
        with pytest.raises(ValueError):
            ev(s, frames, **dict(kw, stabilize=False, inpaint=True))
    for name, out, plain, last, last_mask in runs:
        assert set(out) == set(plain) | new
        for k in plain:
            if k == "pairs":
                assert all(np.array_equal(a[f], b[f]) for a, b in zip(out[k], plain[k]) for f in ("depth_map", "flow", "gs_image"))
            elif k == "path_smoothed":
                assert all(np.array_equal(out[k][f], plain[k][f]) for f in plain[k])
            elif k == "links":
                assert out[k] == plain[k]
            else:
                assert all(np.array_equal(a, b) for a, b in zip(out[k], plain[k])) if isinstance(plain[k], list) else np.array_equal(np.asarray(out[k]), np.asarray(plain[k])), k
        assert out["inpaint_counts"].shape == (4,) and out["inpaint_counts"].dtype == np.int64
        for p in range(4):
            before, src = out[last][p], out["inpaint_sources"][p]
            seen = src != rsdsfm.INPAINT_SOURCE  # (the clip's ids are <= 33)
            if last_mask:
                assert np.array_equal(seen, out[last_mask][p] != 0)
            else:  # the blended mask's set pixels: all but blend_counts' "none"
                assert seen.sum() == rows * cols - out["blend_counts"][p][0]
            assert seen.any()  # there was something to fill from ...
            assert src.all()   # ... so no pixel is left that nobody gave
            assert np.array_equal(out["stab_inpainted"][p][seen], before[seen]) and out["inpaint_counts"][p] == (~seen).sum()
            assert np.array_equal(rsdsfm.formats.read_png(str(tmp_path / name / ("stabilized_inpainted_%d.png" % p))), out["stab_inpainted"][p])
        lines = (tmp_path / name / "inpaint.csv").read_text().strip().split("\n")
        assert lines[0] == "pair,stage,inpainted" and len(lines) == 5
        assert [l.split(",") for l in lines[1:]] == [[str(p), "blended" if name == "full" else "stabilized", str(int(out["inpaint_counts"][p]))] for p in range(4)]
        assert sorted(x.name for x in (tmp_path / (name + "_plain")).iterdir()) == sorted(x.name for x in (tmp_path / name).iterdir() if "inpaint" not in x.name)
    assert runs[1][1]["inpaint_counts"].sum() > 0  # the stabilised frames alone have an empty band
