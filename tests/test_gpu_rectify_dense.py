"""GPU: the dense global-shutter frame (rsdsfm_rectify_dense_frame_dev) bit for bit against its definition (tests/rectify_dense_spec_numpy.py):
filled depth, displacement plane, image and mask.  Inputs as tests/test_gpu_rectify_gray.py's (tests/rectify_dense_cases.py), with a thinned
depth map.  Where the displacement plane holds NaN (a map without a valid pixel, an overflowing depth) the NaNs must sit at the same places;
every other value has the spec's bits."""
import numpy as np
import pytest

import rectify_dense_cases as cases
import rectify_dense_spec_numpy as spec

pytestmark = pytest.mark.gpu

SHAPES = [((2, 2), dict(holes=0.4)),          # the whole pyramid in one cell
          ((5, 3), dict(holes=0.4)),          # smaller than any tile, odd both ways
          ((16, 64), dict(holes=0.4)),        # exactly one tile
          ((33, 68), dict(holes=0.4)),        # ragged tiles, the packed path
          ((33, 70), dict(holes=0.4)),        # the byte tail
          ((150, 200), dict(holes=0.4, block=(30, 60, 40, 50), corner=(12, 17)))]  # several tiles; the push crosses several levels
BIG = SHAPES[-1]
CASES = [(shape, kw, ch, 0, 0, 0) for shape, kw in SHAPES for ch in (3, 1)]
CASES += [((33, 70), dict(holes=0.4), 3, it, 0, 0) for it in (1, 16)]  # (3 is the default: above)
CASES += [((33, 70), dict(holes=0.4), 3, 0, mode, q5) for mode, q5 in ((0, 1), (1, 0))]
CASES += [((33, 70), dict(none_valid=True), ch, 0, 0, 0) for ch in (3, 1)]
CASES += [((33, 70), dict(holes=0.4, specials=True), 3, 0, 0, 0), (BIG[0], dict(BIG[1], specials=True), 1, 0, 0, 0)]

# the large levels: 7 launches (two pulls into the single workgroup's level, two pushes out of it) and 9, the count of a 1280 x 720 frame
LARGE = [((300, 400), dict(holes=0.4, block=(60, 90, 120, 160), corner=(25, 31)), 3, 7),
         ((600, 800), dict(holes=0.5, block=(150, 200, 260, 340), corner=(40, 70), specials=True), 1, 9)]
CASES += [(shape, kw, ch, 0, 0, 0) for shape, kw, ch, _ in LARGE]

_expected = {}


def _case(oracle, shape, kw, ch, it, mode, q5):
    """inputs and the spec's outputs, computed once per case and shared"""
    key = (shape, tuple(sorted(kw.items())), ch, it, mode, q5)
    if key not in _expected:
        rows, cols = shape
        K, image, depth = cases.inputs(rows, cols, channels=ch, **kw)
        R, t = oracle.pose_table(cases.POSE["v"], cases.POSE["w"], cases.POSE["k"], cases.POSE["gamma"], rows)
        R = np.ascontiguousarray(R).reshape(rows, 9)
        _expected[key] = dict(K=K, image=image, depth=depth, R=R, t=t, out=spec.rectify_dense(image, depth, R, t, *K, mode=mode, q5_mode=q5, iterations=it))
    return _expected[key]


def _run(torch, s, e, it, mode, q5):
    """one call with every optional output; the output buffers start as 77 / NaN"""
    dev = torch.device("cuda", 0)
    rows, cols = e["depth"].shape
    ch = 1 if e["image"].ndim == 2 else 3
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_img, d_dm, d_R, d_t = tt(e["image"]), tt(e["depth"].T), tt(e["R"]), tt(e["t"])
    out, mask = torch.full_like(d_img, 77), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
    filled = torch.full((cols, rows), np.nan, dtype=torch.float64, device=dev)
    disp = torch.full((rows, cols, 2), np.nan, dtype=torch.float32, device=dev)
    if not np.isnan(e["out"]["disp"]).any():
        disp.fill_(12345.0)  # (NaN could not tell an unwritten pair from a NaN result)
    torch.cuda.synchronize()
    s.rectify_dense_frame_dev(d_img.data_ptr(), ch, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, out.data_ptr(), mask.data_ptr(),
                              filled.data_ptr(), disp.data_ptr(), mode=mode, q5_mode=q5, iterations=it)
    s.synchronize()
    return dict(image=out.cpu().numpy(), mask=mask.cpu().numpy(), filled=filled.cpu().numpy().T, disp=disp.cpu().numpy())


def _check(got, want):
    assert not np.isnan(got["filled"]).any()  # every double written
    assert np.array_equal(got["filled"].view(np.uint64), want["filled"].view(np.uint64))
    nan = np.isnan(want["disp"])
    assert np.array_equal(np.isnan(got["disp"]), nan)
    assert np.array_equal(got["disp"].view(np.uint32)[~nan], want["disp"].view(np.uint32)[~nan])
    assert np.array_equal(got["mask"], want["mask"])  # (1 or 0: no 77 left)
    assert np.array_equal(got["image"], want["image"])


@pytest.mark.parametrize("shape,kw,ch,it,mode,q5", CASES)
def test_dense_rectifier_equals_the_spec(oracle, rsdsfm, shape, kw, ch, it, mode, q5):
    import torch

    e = _case(oracle, shape, kw, ch, it, mode, q5)
    want = e["out"]
    if kw.get("none_valid"):
        assert not want["image"].any() and not want["mask"].any() and not want["filled"].any()
    elif shape[0] * shape[1] > 64 and mode == 0:
        assert want["mask"].any() and not want["mask"].all() and (want["image"] != e["image"]).any()  # something moved, something left the frame
        if kw.get("specials"):
            assert np.isfinite(want["filled"]).all() and (want["filled"] == 1e308).any()
    with rsdsfm.Solver(0) as s:
        _check(_run(torch, s, e, it, mode, q5), want)


def test_the_large_cases_take_the_large_level_launches(rsdsfm):
    """the cases above that are meant to run rectify_dense_pull_kernel and several rectify_dense_push_kernel launches do"""
    assert [rsdsfm.rectify_dense_launches(*shape) for shape, _, _, _ in LARGE] == [n for _, _, _, n in LARGE]
    assert rsdsfm.rectify_dense_launches(*BIG[0]) == 5 and rsdsfm.rectify_dense_launches(33, 70) == 4


def test_twice_on_one_context_at_two_sizes(oracle, rsdsfm):
    """the workspace is rebuilt when the size changes: A, B, A, B on one context, every result the spec's"""
    import torch

    a = _case(oracle, (33, 70), dict(holes=0.4), 3, 0, 0, 0)
    b = _case(oracle, *BIG, 1, 0, 0, 0)
    with rsdsfm.Solver(0) as s:
        for e in (a, b, a, b):
            _check(_run(torch, s, e, 0, 0, 0), e["out"])


def test_outputs_are_optional_and_fully_written(oracle, rsdsfm):
    """image only: the same bytes, every one of them written (cols % 4 != 0: packed words and the byte tail)"""
    import torch

    dev = torch.device("cuda", 0)
    e = _case(oracle, (33, 70), dict(holes=0.4), 3, 0, 0, 0)
    rows, cols = 33, 70
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_img, d_dm, d_R, d_t = tt(e["image"]), tt(e["depth"].T), tt(e["R"]), tt(e["t"])
    for fill in (77, 0):
        out = torch.full_like(d_img, fill)
        torch.cuda.synchronize()
        with rsdsfm.Solver(0) as s:
            s.rectify_dense_frame_dev(d_img.data_ptr(), 3, d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), e["K"], rows, cols, out.data_ptr())
            s.synchronize()
        assert np.array_equal(out.cpu().numpy(), e["out"]["image"]), fill


def test_host_convenience(oracle, rsdsfm):
    e = _case(oracle, (33, 70), dict(holes=0.4), 3, 0, 0, 0)
    with rsdsfm.Solver(0) as s:
        img, mask = s.rectify_dense(e["image"], e["depth"], e["R"], e["t"], e["K"])
    assert np.array_equal(img, e["out"]["image"]) and np.array_equal(mask, e["out"]["mask"])


def test_argument_errors(rsdsfm):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    img = torch.zeros((rows, cols, 3), dtype=torch.uint8, device=dev)
    out = torch.zeros_like(img)
    dm, R, t = torch.ones(rows * cols, dtype=torch.float64, device=dev), torch.zeros(rows * 9, dtype=torch.float64, device=dev), torch.zeros(rows * 3, dtype=torch.float64, device=dev)
    K = (50.0, 50.0, 32.0, 8.0)
    with rsdsfm.Solver(0) as s:
        call = lambda i=img.data_ptr(), ch=3, d=dm.data_ptr(), o=out.data_ptr(), r=rows, c=cols, **kw: s.rectify_dense_frame_dev(
            i, ch, d, R.data_ptr(), t.data_ptr(), K, r, c, o, **kw)
        for bad in (dict(o=img.data_ptr()),  # aliased in and out
                    dict(o=0), dict(i=0), dict(d=0), dict(ch=2), dict(mode=2), dict(q5_mode=7), dict(iterations=17), dict(iterations=-1),
                    dict(r=1), dict(c=1), dict(c=16385), dict(o=out.data_ptr() + 1)):
            with pytest.raises(rsdsfm.RsdsfmError):
                call(**bad)
        call()  # the same arguments without a fault go through
        s.synchronize()


def test_destroy_releases_the_workspace(rsdsfm):
    """create / dense call at two sizes / destroy, 12 times at 1280 x 720 (9.8 MB of workspace each): the device's free memory does not go down
    by a leak's 118 MB.  Free memory is device-wide and other processes share the device, so a step larger than 40 MB is measured again, up
    to three times: a leak shows every time."""
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 720, 1280
    img = torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
    out = torch.zeros_like(img)
    dm, R, t = torch.ones(rows * cols, dtype=torch.float64, device=dev), torch.zeros(rows * 9, dtype=torch.float64, device=dev), torch.zeros(rows * 3, dtype=torch.float64, device=dev)
    K = (1000.0, 1000.0, 640.0, 360.0)

    def cycle():
        with rsdsfm.Solver(0) as s:
            for r, c in ((rows, cols), (100, 200), (rows, cols)):
                s.rectify_dense_frame_dev(img.data_ptr(), 1, dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, r, c, out.data_ptr())
            s.synchronize()

    cycle()
    steps = []
    for _ in range(3):
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        for _ in range(12):
            cycle()
        steps.append((before - torch.cuda.mem_get_info()[0]) / 1e6)
        if steps[-1] < 40.0:
            break
    assert min(steps) < 40.0, steps
