"""GPU: the synthetic shutter (include/rsdsfm_shutter.h) bit for bit against its definition (tests/shutter_spec_numpy.py) in both library builds
-- the accumulate alone at the shapes where its kernel can go wrong, the divide over every (s, n), the frame call on every case of
tests/shutter_cases.py against the golden fixture the CPU suite holds to the definition and against the public calls made one after another,
argument errors -- and the clip call on a clip of three sources against the frame calls made one after another."""
import os

import numpy as np
import pytest

import shutter_cases as cases
import shutter_spec_numpy as spec

pytestmark = pytest.mark.gpu

GUARD = 0xCD
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_shutter_v1.npz")


def _guarded(torch, dev, a):
    """a's bytes on the device with 16 guard bytes behind them: (the view of a's shape, the guard)"""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + 16,), GUARD, dtype=torch.uint8, device=dev)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[:a.size].view(*a.shape), buf[a.size:]


def _outputs(torch, dev, image_shape, plane_shape):
    """the three output planes, never preset (every byte GUARD, and 16 guard bytes behind each), and the counters with a guard on either side"""
    planes = [_guarded(torch, dev, np.full(shape, GUARD, dtype=np.uint8)) for shape in (image_shape, plane_shape, plane_shape)]
    return planes, torch.full((5,), -1, dtype=torch.int64, device=dev)


def _collect(planes, cnt, guards=(), with_coverage=True, with_counts=True):
    for g in [p[1] for p in planes] + list(guards):
        assert (g.cpu().numpy() == GUARD).all()
    c = cnt.cpu().numpy().tolist()
    assert c[0] == -1 and c[4] == -1 and (with_counts or c[1:4] == [-1] * 3)
    (d_img, _), (d_mask, _), (d_cov, _) = planes
    coverage = d_cov.cpu().numpy()
    assert with_coverage or (coverage == GUARD).all()
    return dict(image=d_img.cpu().numpy(), mask=d_mask.cpu().numpy(), coverage=coverage, counts=c[1:4])


def _same(got, want, name="", coverage=True, counts=True):
    for k in ("image", "mask") + (("coverage",) if coverage else ()):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert not counts or list(got["counts"]) == list(want["counts"]), (name, got["counts"], want["counts"])


def _cells(torch, dev, rows, cols, channels, value=0xFFFF):
    """rows x cols cells preset to `value` in every uint16 (what `first` must overwrite), 16 guard bytes behind them: (cells as bytes, guard)"""
    a = np.full((rows, cols, channels + 1), value, dtype=np.uint16)
    return _guarded(torch, dev, a.view(np.uint8))


def _cells_host(d_cells, rows, cols, channels):
    return d_cells.cpu().numpy().view(np.uint16).reshape(rows, cols, channels + 1)


def _expose(torch, s, samples, min_samples=1, with_coverage=True, with_counts=True, last_again=None):
    """the samples through rsdsfm_shutter_accumulate_dev one after another on guarded planes, the cells preset to 0xFFFF and the outputs never
    preset.  -> (the collected outputs, the cells as the last launch left them); last_again: a second min_samples, for which only the last
    launch is made once more (it does not write the cells), its outputs collected too"""
    dev = torch.device("cuda", 0)
    rows, cols = samples[0][1].shape
    ch = 1 if samples[0][0].ndim == 2 else 3
    S = len(samples)
    d_s = [(_guarded(torch, dev, i), _guarded(torch, dev, m)) for i, m in samples]
    d_cells, cells_guard = _cells(torch, dev, rows, cols, ch)
    planes, cnt = _outputs(torch, dev, samples[0][0].shape, (rows, cols))
    torch.cuda.synchronize()

    def launch(j, need, planes, cnt):
        (d_i, _), (d_m, _) = d_s[j]
        s.shutter_accumulate_dev(d_i.data_ptr(), d_m.data_ptr(), ch, rows, cols, d_cells.data_ptr(), j == 0, j == S - 1, S, need, planes[0][0].data_ptr(),
                                 planes[1][0].data_ptr(), planes[2][0].data_ptr() if with_coverage else None, cnt[1:].data_ptr() if with_counts else None)

    for j in range(S):
        launch(j, min_samples, planes, cnt)
    s.synchronize()
    guards = [g for (_, gi), (_, gm) in d_s for g in (gi, gm)] + [cells_guard]
    for ((d_i, _), (d_m, _)), (i, m) in zip(d_s, samples):  # the samples are only read
        assert np.array_equal(d_i.cpu().numpy(), i) and np.array_equal(d_m.cpu().numpy(), m)
    got = _collect(planes, cnt, guards, with_coverage, with_counts)
    cells = _cells_host(d_cells, rows, cols, ch).copy()
    if last_again is None:
        return got, cells
    planes2, cnt2 = _outputs(torch, dev, samples[0][0].shape, (rows, cols))
    torch.cuda.synchronize()
    launch(S - 1, last_again, planes2, cnt2)
    s.synchronize()
    assert np.array_equal(_cells_host(d_cells, rows, cols, ch), cells)
    return got, cells, _collect(planes2, cnt2, [cells_guard], with_coverage, with_counts)


def _spec_cells(samples, upto):
    """the definition's cells after the first `upto` samples"""
    cells = None
    for j in range(upto):
        cells = spec.accumulate(cells, samples[j][0], samples[j][1], j == 0)
    return cells


# ---------------------------------------------------------------------------------------------------
# the accumulate
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["reference", "fused"])
@pytest.mark.parametrize("channels", [1, 3])
def test_the_accumulate_equals_the_definition(rsdsfm, arith, channels):
    """every shape (one word, byte tails of 1 and 3, more than one workgroup), S in {1, 2, 3, 64}, min_samples in {1, S}; masks with empty, full
    and mixed words and values other than 0 / 1 at a different phase per sample, random bytes under empty mask bytes; `first` on cells preset
    to 0xFFFF; the cells after the last launch are the definition's after S - 1 samples (the last launch does not write them; with S = 1 they
    keep the preset); counters and coverage; guard bytes behind every plane"""
    import torch

    seen = np.zeros(3, dtype=np.int64)
    with rsdsfm.Solver(0, arith=arith) as s:
        for shape in cases.ACC_SHAPES:
            for S in cases.ACC_SAMPLES:
                ss = cases.samples(*shape, channels, S)
                got, cells, got_all = _expose(torch, s, ss, 1, last_again=S)
                want_one, want_all = spec.expose(ss, 1), spec.expose(ss, S)
                _same(got, want_one, (shape, S, 1))
                _same(got_all, want_all, (shape, S, S))
                want_cells = _spec_cells(ss, S - 1) if S > 1 else np.full(shape + (channels + 1,), 0xFFFF, dtype=np.uint16)
                assert np.array_equal(cells, want_cells), (shape, S)
                seen += np.array(want_one["counts"]) + np.array(want_all["counts"])
            ss = cases.samples(*shape, channels, 3, seed=1)
            want = spec.expose(ss, 2)
            for with_coverage, with_counts in ((False, True), (True, False), (False, False)):
                _same(_expose(torch, s, ss, 2, with_coverage, with_counts)[0], want, shape, with_coverage, with_counts)
        assert rsdsfm.shutter_accumulate_launches() == 1
    assert (seen > 0).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_saturation_order_and_untouched_cells(rsdsfm, channels):
    """64 samples of 255, all set: the largest sums; a permuted sample order gives the same bytes; a mid sample leaves the cells of its empty
    mask words byte for byte as they were and adds to the others"""
    import torch

    dev = torch.device("cuda", 0)
    with rsdsfm.Solver(0) as s:
        ss = cases.saturated(16, 131, channels)
        got, cells = _expose(torch, s, ss)
        _same(got, spec.expose(ss))
        assert (got["image"] == 255).all() and (got["coverage"] == 64).all() and got["counts"] == [0, 0, 16 * 131]
        assert (cells[..., :-1] == 63 * 255).all() and (cells[..., -1] == 63).all()

        ss = cases.samples(37, 67, channels, 9)
        want = spec.expose(ss, 3)
        _same(_expose(torch, s, ss, 3)[0], want)
        for seed in (1, 2):
            order = np.random.default_rng(seed).permutation(9)
            _same(_expose(torch, s, [ss[i] for i in order], 3)[0], want, ("order", seed))

        # a mid sample on cells that hold valid sums: neither first nor last
        rows, cols = 37, 67
        rng = np.random.default_rng(5)
        n0 = rng.integers(0, 4, size=(rows, cols, 1))
        before = np.concatenate([rng.integers(0, 256, size=(rows, cols, channels)) * n0, n0], axis=-1).astype(np.uint16)
        d_cells, guard = _guarded(torch, dev, before.view(np.uint8))
        image, mask = ss[4]
        (d_i, gi), (d_m, gm) = _guarded(torch, dev, image), _guarded(torch, dev, mask)
        torch.cuda.synchronize()
        s.shutter_accumulate_dev(d_i.data_ptr(), d_m.data_ptr(), channels, rows, cols, d_cells.data_ptr(), False, False, 9)
        s.synchronize()
        after = _cells_host(d_cells, rows, cols, channels)
        assert np.array_equal(after, spec.accumulate(before, image, mask, False))
        empty_words = (mask.reshape(-1)[:rows * cols // 4 * 4].reshape(-1, 4) == 0).all(axis=1)
        assert empty_words.sum() > 50
        flat = lambda a: a.reshape(-1, channels + 1)[:rows * cols // 4 * 4].reshape(-1, 4 * (channels + 1))
        assert np.array_equal(flat(after)[empty_words], flat(before)[empty_words])
        for g in (guard, gi, gm):
            assert (g.cpu().numpy() == GUARD).all()


def test_the_divide_for_every_sum_and_count(rsdsfm):
    """every (s, n) with n in 1 .. 64 and s <= 255 n as the pixels of one gray frame exposed from 64 samples: the kernel's divide is
    (2 s + n) // (2 n) on each of the 530 464 pairs"""
    import torch

    dev = torch.device("cuda", 0)
    ss, s_, n_ = cases.division_pairs()
    rows, cols = ss[0][1].shape
    d_s = [(torch.from_numpy(i).to(dev), torch.from_numpy(m).to(dev)) for i, m in ss]
    d_cells = torch.empty((rows, cols, 2), dtype=torch.int16, device=dev)
    d_out, d_mask, d_cov = (torch.empty((rows, cols), dtype=torch.uint8, device=dev) for _ in range(3))
    d_cnt = torch.zeros(3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        for j, (d_i, d_m) in enumerate(d_s):
            s.shutter_accumulate_dev(d_i.data_ptr(), d_m.data_ptr(), 1, rows, cols, d_cells.data_ptr(), j == 0, j == 63, 64, 1, d_out.data_ptr(), d_mask.data_ptr(),
                                     d_cov.data_ptr(), d_cnt.data_ptr())
        s.synchronize()
    assert np.array_equal(d_cov.cpu().numpy().reshape(-1), n_) and (d_mask.cpu().numpy() == 1).all()
    assert np.array_equal(d_out.cpu().numpy().reshape(-1), (2 * s_ + n_) // (2 * n_))
    assert d_cnt.cpu().numpy().tolist() == [0, int((n_ < 64).sum()), int((n_ == 64).sum())]


def test_the_host_convenience_of_the_accumulate(rsdsfm):
    ss = cases.samples(37, 67, 3, 5)
    want = spec.expose(ss, 2)
    with rsdsfm.Solver(0) as s:
        img, mask, cov, counts = s.shutter_accumulate(ss, min_samples=2)
    _same(dict(image=img, mask=mask, coverage=cov, counts=counts.tolist()), want)


def test_accumulate_argument_errors(rsdsfm):
    """every refusal returns RSDSFM_ERR_INVALID and enqueues nothing: the outputs and the cells keep their sentinel; after each refused call the
    same call without the fault goes through"""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    u8 = lambda value, *shape: torch.full(shape, value, dtype=torch.uint8, device=dev)
    img, mask = u8(9, rows, cols, 3), u8(1, rows, cols)
    out, omask, cov = u8(GUARD, rows, cols + 4, 3), u8(GUARD, rows, cols + 4), u8(GUARD, rows, cols + 4)
    cells = torch.full((rows, cols + 4, 4), 0x7BCD, dtype=torch.int16, device=dev)
    counts = torch.full((5,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        def acc(i=img.data_ptr(), m=mask.data_ptr(), ch=3, r=rows, c=cols, cl=cells.data_ptr(), first=1, last=1, n=4, need=2, o=out.data_ptr(), k=omask.data_ptr(),
                cv=cov.data_ptr(), cnt=counts[1:].data_ptr()):
            return s.shutter_accumulate_dev(i, m, ch, r, c, cl, first, last, n, need, o, k, cv, cnt)

        bads = (dict(i=0), dict(m=0), dict(o=0), dict(k=0), dict(cl=0, first=0), dict(cl=0, last=0), dict(i=img.data_ptr() + 1), dict(m=mask.data_ptr() + 2),
                dict(o=out.data_ptr() + 1), dict(k=omask.data_ptr() + 2), dict(cv=cov.data_ptr() + 3), dict(cl=cells.data_ptr() + 4), dict(cnt=counts.data_ptr() + 4),
                dict(o=img.data_ptr()), dict(k=mask.data_ptr()), dict(cv=img.data_ptr()), dict(o=cells.data_ptr()), dict(k=out.data_ptr()), dict(cv=omask.data_ptr()),
                dict(cv=out.data_ptr()), dict(cl=img.data_ptr()), dict(m=img.data_ptr()), dict(ch=2), dict(ch=4), dict(r=1), dict(c=16385), dict(r=16385), dict(c=1),
                dict(first=2), dict(last=-1), dict(n=0), dict(n=65), dict(need=0), dict(need=5), dict(n=1, need=2))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                acc(**bad)
        s.synchronize()
        for x in (out, omask, cov):  # nothing was enqueued
            assert (x.cpu().numpy() == GUARD).all()
        assert (cells.cpu().numpy().view(np.uint16) == 0x7BCD).all() and counts.cpu().numpy().tolist() == [-1] * 5
        for bad in bads[:3]:
            with pytest.raises(rsdsfm.RsdsfmError):
                acc(**bad)
            acc()  # the same call without the fault goes through
        acc(cl=0)  # first and last: the cells may be NULL
        s.synchronize()
        assert counts.cpu().numpy().tolist() == [-1, rows * cols, 0, 0, -1]  # one sample of four, two needed: every pixel is unset
        assert (out.cpu().numpy().reshape(-1)[:rows * cols * 3] == 0).all() and (omask.cpu().numpy().reshape(-1)[:rows * cols] == 0).all()
        acc(n=1, need=1, cv=None, cnt=None)
        s.synchronize()
        flat = out.cpu().numpy().reshape(-1)
        assert (flat[:rows * cols * 3] == 9).all() and (flat[rows * cols * 3:] == GUARD).all() and (omask.cpu().numpy().reshape(-1)[:rows * cols] == 1).all()
        # not last: the outputs are not read -- NULL and misaligned ones pass, and nothing is written to them
        acc(last=0, o=0, k=0, cv=0, cnt=0)
        acc(last=0, first=0, o=out.data_ptr() + 1, k=3, cv=5, cnt=counts.data_ptr() + 4)
        s.synchronize()
        c16 = cells.cpu().numpy().view(np.uint16).reshape(-1)[:rows * cols * 4].reshape(-1, 4)
        assert (c16 == [18, 18, 18, 2]).all() and counts.cpu().numpy().tolist() == [-1, rows * cols, 0, 0, -1]


# ---------------------------------------------------------------------------------------------------
# the frame call
# ---------------------------------------------------------------------------------------------------
def _clip(torch, dev, case):
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(frames=[tt(x) for x in case["frames"]], maps=[tt(z.T) for z in case["depths"]], Rs=[tt(np.asarray(R).reshape(-1, 9)) for R in case["Rs"]],
                ts=[tt(t) for t in case["ts"]])


def _clip_args(d, case):
    rows, cols = case["depths"][0].shape
    ptrs = lambda a: [x.data_ptr() for x in a]
    return (ptrs(d["frames"]), rows, cols, 1 if case["frames"][0].ndim == 2 else 3, case["K"], ptrs(d["maps"]), ptrs(d["Rs"]), ptrs(d["ts"]), case["A"], case["c"],
            case["A_path"], case["c_path"], case["scales"])


def _render_kw(case):
    return dict(window=case["window"], threshold=case["threshold"], occlusion=case["occlusion"], occlusion_tol_q16=case["tol_q16"], mode=case["mode"],
                q5_mode=case["q5_mode"], iterations=case["iterations"])


def _frame(torch, s, case, with_coverage=True, with_counts=True):
    """one rsdsfm_shutter_frame_dev of a case (the context's knob set to the case's) into guarded, never preset outputs -> (outputs, kept)"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    d = _clip(torch, dev, case)
    planes, cnt = _outputs(torch, dev, case["frames"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    s.set_occlusion_search(case["search"])
    kept = s.shutter_frame_dev(*_clip_args(d, case), case["t"], planes[0][0].data_ptr(), planes[1][0].data_ptr(), planes[2][0].data_ptr() if with_coverage else None,
                               cnt[1:].data_ptr() if with_counts else None, shutter=case["shutter"], samples=case["samples"], min_samples=case["min_samples"],
                               **_render_kw(case))
    s.synchronize()
    s.set_occlusion_search(0)
    return _collect(planes, cnt, (), with_coverage, with_counts), kept


def _parts(torch, rsdsfm, s, case):
    """the public calls one after another: shutter_times, then per kept sub-instant retime_poses, rsdsfm_retime_frame_dev into planes of the
    test's own and rsdsfm_shutter_accumulate_dev on cells of the test's own"""
    dev = torch.device("cuda", 0)
    rows, cols = case["depths"][0].shape
    ch = 1 if case["frames"][0].ndim == 2 else 3
    ns = len(case["depths"])
    d = _clip(torch, dev, case)
    d_simg, d_smask = torch.full_like(d["frames"][0], 99), torch.full((rows, cols), 99, dtype=torch.uint8, device=dev)
    d_cells = torch.full((rows, cols, ch + 1), -1, dtype=torch.int16, device=dev)
    planes, cnt = _outputs(torch, dev, case["frames"][0].shape, (rows, cols))
    torch.cuda.synchronize()
    times = rsdsfm.shutter_times(case["t"], case["shutter"], case["samples"], ns)
    s.set_occlusion_search(case["search"])
    for j, tj in enumerate(times):
        src, w, M, m, _, _ = rsdsfm.retime_poses(case["A"], case["c"], case["A_path"], case["c_path"], case["scales"], tj, nsources=ns)
        s.retime_frame_dev([d["frames"][q].data_ptr() for q in src], ch, [d["maps"][q].data_ptr() for q in src], [d["Rs"][q].data_ptr() for q in src],
                           [d["ts"][q].data_ptr() for q in src], case["K"], rows, cols, M, m, w, d_simg.data_ptr(), d_smask.data_ptr(), **_render_kw(case))
        s.shutter_accumulate_dev(d_simg.data_ptr(), d_smask.data_ptr(), ch, rows, cols, d_cells.data_ptr(), j == 0, j == len(times) - 1, len(times),
                                 min(case["min_samples"], len(times)), planes[0][0].data_ptr(), planes[1][0].data_ptr(), planes[2][0].data_ptr(), cnt[1:].data_ptr())
    s.synchronize()
    s.set_occlusion_search(0)
    return _collect(planes, cnt), len(times)


@pytest.mark.parametrize("arith", ["reference", "fused"])
def test_every_case_equals_the_definition_and_the_public_calls(oracle, rsdsfm, arith):
    """image, mask, coverage, the three counts and the kept count of every fixture case -- the shift scene, a fold pair through the occlusion test
    and through the search, smooth clips of three sources, a zoomed window, the 2 x 2 dense case, windows clipped at t = 0 and at the end, an
    integer t, the identity forms -- against the golden fixture, and against the public calls made one after another"""
    import torch

    g = np.load(GOLDEN)
    with rsdsfm.Solver(0, arith=arith) as s:
        for case in cases.all_cases(oracle.pose_table):
            n = case["name"] + "/"
            want = dict(image=g[n + "image"], mask=g[n + "mask"], coverage=g[n + "coverage"], counts=g[n + "counts"].tolist())
            got, kept = _frame(torch, s, case)
            _same(got, want, case["name"])
            assert kept == len(g[n + "times"]), case["name"]
            parts, kept_parts = _parts(torch, rsdsfm, s, case)
            _same(parts, want, (case["name"], "parts"))
            assert kept_parts == kept
        case = cases.fold_clip(37, 67, 3, 1, 0)
        want = cases.run_spec(case)
        for with_coverage, with_counts in ((False, True), (True, False), (False, False)):
            _same(_frame(torch, s, case, with_coverage, with_counts)[0], want, "optional", with_coverage, with_counts)


def test_the_identity_forms_equal_the_retime_frame_call(rsdsfm):
    """shutter = 0 with S = 5, and S = 1 with a wide shutter: rsdsfm_retime_frame_dev's image bytes and its mask, on the device"""
    import torch

    dev = torch.device("cuda", 0)
    with rsdsfm.Solver(0) as s:
        for case in (cases.smooth_clip(33, 70, 3, 6, t=0.7, shutter=0.0, samples=5), cases.smooth_clip(33, 70, 1, 7, t=0.7, shutter=0.9, samples=1),
                     cases.fold_clip(24, 40, 3, 1, 0, t=0.5, shutter=0.0, samples=64, min_samples=64), cases.smooth_clip(33, 70, 3, 8, t=1.0, shutter=0.0, samples=2)):
            got, kept = _frame(torch, s, case)
            assert kept == case["samples"]
            rows, cols = case["depths"][0].shape
            ch = 1 if case["frames"][0].ndim == 2 else 3
            d = _clip(torch, dev, case)
            d_img, d_mask = torch.full_like(d["frames"][0], 7), torch.full((rows, cols), 7, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            src, w, M, m, _, _ = rsdsfm.retime_poses(case["A"], case["c"], case["A_path"], case["c_path"], case["scales"], case["t"], nsources=len(case["depths"]))
            s.retime_frame_dev([d["frames"][q].data_ptr() for q in src], ch, [d["maps"][q].data_ptr() for q in src], [d["Rs"][q].data_ptr() for q in src],
                               [d["ts"][q].data_ptr() for q in src], case["K"], rows, cols, M, m, w, d_img.data_ptr(), d_mask.data_ptr(), **_render_kw(case))
            s.synchronize()
            assert np.array_equal(got["image"], d_img.cpu().numpy()) and np.array_equal(got["mask"], d_mask.cpu().numpy()), case["name"]
            assert np.array_equal(got["coverage"], d_mask.cpu().numpy() * case["samples"])


def test_the_shift_scene_is_the_analytic_mean_on_the_device(rsdsfm):
    """t = 0.5625, shutter 0.5, S = 4: every pixel is (2 sum_{k = 3 .. 6} base[y, (x + k) mod 16] + 4) // 8, full 960, partial 0, unset 0"""
    import torch

    base = cases.shift_base().astype(np.int64)
    x = np.arange(40)
    want = (2 * sum(base[:, (x + k) % 16] for k in (3, 4, 5, 6)) + 4) // 8
    with rsdsfm.Solver(0) as s:
        got, kept = _frame(torch, s, cases.shift_clip())
    assert kept == 4 and np.array_equal(got["image"], want) and (got["mask"] == 1).all() and (got["coverage"] == 4).all() and got["counts"] == [0, 0, 960]


def test_frame_argument_errors(rsdsfm):
    """a refused frame call enqueues nothing: the outputs keep their sentinel"""
    import torch

    dev = torch.device("cuda", 0)
    case = cases.smooth_clip(16, 64, 3, 9, t=1.0, shutter=0.5, samples=4)
    rows, cols = 16, 64
    d = _clip(torch, dev, case)
    out = torch.full((rows, cols + 4, 3), GUARD, dtype=torch.uint8, device=dev)
    mask, cov = (torch.full((rows, cols + 4), GUARD, dtype=torch.uint8, device=dev) for _ in range(2))
    counts = torch.full((5,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    args = list(_clip_args(d, case))
    nanA = case["A"].copy()
    nanA[1, 0, 0] = np.nan
    bad_bytes = rsdsfm.ShutterParams()
    bad_bytes.shutter, bad_bytes.samples, bad_bytes.min_samples, bad_bytes.struct_bytes = 0.5, 4, 1, 16
    with rsdsfm.Solver(0) as s:
        def frame(t=1.0, o=out.data_ptr(), k=mask.data_ptr(), cv=cov.data_ptr(), cnt=counts[1:].data_ptr(), replace=None, **kw):
            a = list(args)
            for i, v in (replace or {}).items():
                a[i] = v
            kw.setdefault("shutter", 0.5)
            kw.setdefault("samples", 4)
            return s.shutter_frame_dev(*a, t, o, k, cv, cnt, **kw)

        bads = (dict(t=-0.1), dict(t=2.5), dict(t=np.nan), dict(shutter=-0.5), dict(shutter=2.5), dict(shutter=np.inf), dict(samples=0), dict(samples=65),
                dict(min_samples=0), dict(min_samples=5), dict(shutter_params=bad_bytes), dict(o=0), dict(k=0), dict(o=out.data_ptr() + 2), dict(cv=cov.data_ptr() + 1),
                dict(cnt=counts.data_ptr() + 4), dict(k=out.data_ptr()), dict(cv=mask.data_ptr()), dict(o=args[0][1]), dict(replace={0: [args[0][0], 0, args[0][2]]}),
                dict(replace={5: [0] + args[5][1:]}), dict(replace={3: 2}), dict(replace={1: 1}), dict(replace={8: nanA}), dict(replace={12: [1.0, -1.0, 1.0]}),
                dict(threshold=256), dict(occlusion=2), dict(window=(0, 0, 0, 8)), dict(iterations=17), dict(mode=2))
        for bad in bads:
            with pytest.raises(rsdsfm.RsdsfmError):
                frame(**bad)
        s.synchronize()
        for x in (out, mask, cov):  # nothing was enqueued
            assert (x.cpu().numpy() == GUARD).all()
        assert counts.cpu().numpy().tolist() == [-1] * 5
        assert frame() == 4 and frame(t=0.0) == 2  # and the same call without a fault goes through
        s.synchronize()
        assert sum(counts.cpu().numpy().tolist()[1:4]) == rows * cols


# ---------------------------------------------------------------------------------------------------
# the clip call
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
def test_the_clip_call_equals_the_frame_calls(rsdsfm, channels):
    """a clip of three sources of 33 x 70 frames at the instants [0, 0.5, 1, 1.3, 2]: every plane and host array of rsdsfm_shutter_video_dev is byte
    for byte rsdsfm_shutter_frame_dev made once per instant, with and without the counts; a refused time enqueues nothing; the launches are
    shutter_launches' of the kept sub-instants"""
    import torch

    dev = torch.device("cuda", 0)
    case = cases.smooth_clip(33, 70, channels, 11, t=0.0, shutter=0.8, samples=5, min_samples=2)
    rows, cols, ns = 33, 70, 3
    times = [0.0, 0.5, 1.0, 1.3, 2.0]
    nt = len(times)
    d = _clip(torch, dev, case)
    image = lambda value: [torch.full_like(d["frames"][0], value) for _ in range(nt)]
    plane = lambda value: [torch.full((rows, cols), value, dtype=torch.uint8, device=dev) for _ in range(nt)]
    d_out, d_mask, d_cov = image(GUARD), plane(GUARD), plane(GUARD)
    d_one, d_onemask, d_onecov = image(55), plane(55), plane(55)
    d_cnt = torch.zeros((nt, 3), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ptrs = lambda a: [x.data_ptr() for x in a]
    kw = dict(shutter=case["shutter"], samples=case["samples"], min_samples=case["min_samples"])
    with rsdsfm.Solver(0) as s:
        clip = _clip_args(d, case)
        for bad in ([0.0, 0.5, 2.5], [0.0, np.nan], [-0.25]):
            with pytest.raises(rsdsfm.RsdsfmError):
                s.shutter_video_dev(*clip, bad, ptrs(d_out), ptrs(d_mask), ptrs(d_cov), **kw)
        with pytest.raises(rsdsfm.RsdsfmError):
            s.shutter_video_dev(*clip, times, ptrs(d_out), ptrs(d_mask), ptrs(d_cov), shutter=2.5, samples=5)
        s.synchronize()
        assert all((x.cpu().numpy() == GUARD).all() for x in d_out + d_mask + d_cov)  # nothing was enqueued
        got = s.shutter_video_dev(*clip, times, ptrs(d_out), ptrs(d_mask), ptrs(d_cov), **kw)
        s.synchronize()
        kept = [s.shutter_frame_dev(*clip, t, d_one[i].data_ptr(), d_onemask[i].data_ptr(), d_onecov[i].data_ptr(), d_cnt[i].data_ptr(), **kw) for i, t in enumerate(times)]
        s.synchronize()
        assert got["kept"].tolist() == kept == [len(spec.shutter_times(t, case["shutter"], case["samples"], ns)) for t in times] and kept[0] < 5 and kept[2] == 5
        assert got["counts"].tobytes() == d_cnt.cpu().numpy().tobytes() and (got["counts"].sum(axis=1) == rows * cols).all()
        for i in range(nt):
            for a, b in ((d_out, d_one), (d_mask, d_onemask), (d_cov, d_onecov)):
                assert np.array_equal(a[i].cpu().numpy(), b[i].cpu().numpy()), (i, times[i])
            want = cases.run_spec(dict(case, t=times[i]))
            _same(dict(image=d_out[i].cpu().numpy(), mask=d_mask[i].cpu().numpy(), coverage=d_cov[i].cpu().numpy(), counts=got["counts"][i].tolist()), want, times[i])
            sub = spec.shutter_times(times[i], case["shutter"], case["samples"], ns)
            n1 = sum(1 for t in sub if t == np.floor(t))
            assert rsdsfm.shutter_launches(rows, cols, n1, len(sub) - n1) == n1 * rsdsfm.retime_launches(rows, cols, 1) + (len(sub) - n1) * rsdsfm.retime_launches(rows, cols, 2) + len(sub)
        # without the counts and the coverage planes the call only enqueues: the same planes
        again = s.shutter_video_dev(*clip, times, ptrs(d_one), ptrs(d_onemask), want_counts=False, **kw)
        s.synchronize()
        assert "counts" not in again and again["kept"].tolist() == kept
        for i in range(nt):
            assert np.array_equal(d_out[i].cpu().numpy(), d_one[i].cpu().numpy()) and np.array_equal(d_mask[i].cpu().numpy(), d_onemask[i].cpu().numpy())


def test_shutter_and_retime_calls_alternate_on_one_context(rsdsfm):
    """shutter at one size -> retime -> shutter at another size -> shutter at the first again, on ONE context: the sample planes and the cells come
    with the first call and again after the size change, and do not disturb the retimer's layers"""
    import torch

    from test_gpu_retime import _frame as retime_frame
    from test_gpu_retime import _same as retime_same
    import retime_cases as rcases

    a, b = cases.fold_clip(37, 67, 3, 1, 1, t=0.4, shutter=0.6, samples=4), cases.smooth_clip(33, 70, 1, 4, t=1.0, shutter=1.0, samples=3)
    two = rcases.fold_pair(37, 67, 3, 1, 1)
    with rsdsfm.Solver(0) as s:
        _same(_frame(torch, s, a)[0], cases.run_spec(a), "first size")
        retime_same(retime_frame(torch, s, two), rcases.run_spec(two), "retime between")
        _same(_frame(torch, s, b)[0], cases.run_spec(b), "another size")
        _same(_frame(torch, s, a)[0], cases.run_spec(a), "the first size again")


def test_evaluate_real_sequence_with_shutter(rsdsfm, tmp_path):
    """evaluate_real_sequence(..., stabilize=True, retime=2, shutter=(0.5, 4)) adds exactly shuttered, shutter_masks, shutter_coverage,
    shutter_counts, shutter_kept and the files shuttered_<i>.png and shutter.csv; the retimed keys and files are what they were"""
    from test_gpu_stabilize_search import plain_clip

    frames, rows, cols, K, gamma, seeds, _ = plain_clip(rsdsfm)
    ev = rsdsfm.evaluate.evaluate_real_sequence
    kw = dict(camera=K, gamma=gamma, trials=20, seeds=seeds, stabilize=True, smooth_sigma=1.0, retime=2)
    n = len(frames) - 1
    with rsdsfm.Solver(0) as s:
        out = ev(s, frames, shutter=(0.5, 4), out_dir=str(tmp_path / "with"), **kw)
        plain = ev(s, frames, out_dir=str(tmp_path / "without"), **kw)
        zero = ev(s, frames, shutter=0.0, **kw)
    new = {"shuttered", "shutter_masks", "shutter_coverage", "shutter_counts", "shutter_kept"}
    assert set(out) == set(plain) | new
    nt = len(out["retime_times"])
    assert nt == 2 * (n - 1) + 1 and all(len(out[k]) == nt for k in ("shuttered", "shutter_masks", "shutter_coverage"))
    assert out["shutter_counts"].shape == (nt, 3) and (out["shutter_counts"].sum(axis=1) == rows * cols).all()
    assert out["shutter_kept"].tolist() == [len(spec.shutter_times(t, 0.5, 4, n)) for t in out["retime_times"]]
    for k in plain:  # the retimed keys included
        if k not in ("pairs", "path_smoothed", "links"):
            assert np.asarray(out[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    for i in range(nt):  # shutter = 0 with the default eight samples: the retimed frame
        assert np.array_equal(zero["shuttered"][i], plain["retimed"][i]) and np.array_equal(zero["shutter_masks"][i], plain["retime_masks"][i]), i
        assert out["shuttered"][i].shape == frames[0].shape and out["shutter_coverage"][i].max() <= out["shutter_kept"][i]
    with_files, without_files = set(os.listdir(str(tmp_path / "with"))), set(os.listdir(str(tmp_path / "without")))
    assert with_files == without_files | {"shuttered_%d.png" % i for i in range(nt)} | {"shutter.csv"}
    for name in [f for f in without_files if f.startswith("retime")]:
        assert open(str(tmp_path / "with" / name), "rb").read() == open(str(tmp_path / "without" / name), "rb").read(), name
    lines = open(str(tmp_path / "with" / "shutter.csv")).read().split()
    assert lines[0] == "index,time,kept,unset,partial,full" and len(lines) == 1 + nt
    assert lines[2] == ",".join(["1", "0.5", str(int(out["shutter_kept"][1]))] + [str(int(x)) for x in out["shutter_counts"][1]])
