"""GPU: the one-channel rectifier (rsdsfm_rectify_gray_frame_dev).  A gray value g is the BGR pixel (g, g, g); every output is compared
bit for bit with the oracle on the replicated image, channel 0 taken (tests/test_rectify_video_cpu.py shows the channels are equal)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(16, 64, 0),        # exactly one claim tile and one write tile, no inliers
          (33, 68, 5000),     # ragged tiles, cols % 4 == 0: the packed fast path
          (33, 70, 5000),     # cols % 4 != 0: three launches, unaligned rows
          (5, 3, 10),         # smaller than any tile, 15 pixels: the byte-wise tail
          (150, 200, 40000)]  # colliding inliers, several tiles each way
# offsets 1 and 2 everywhere; 3 forces three launches on a cols % 4 == 0 image; the modes at one shape
CASES = [(r, c, m, off, 0, 0) for r, c, m in SHAPES for off in (1, 2)] + [(33, 68, 5000, 3, 0, 0)] + [(33, 68, 5000, 1, mode, q5) for mode, q5 in ((0, 1), (1, 0))]


def _inputs(rsdsfm, rows, cols, m):
    """as tests/test_gpu_rectify.py::test_rectify_frame_one_call_equals_the_oracle, with a gray image: 2 % marker pixels, 5 % values 0..8"""
    rng = np.random.default_rng(rows * 7 + cols)
    K = (0.8 * cols, 0.8 * cols, cols / 2.0 - 0.3, rows / 2.0 + 0.2)
    g = rng.integers(16, 256, size=(rows, cols), dtype=np.uint8)
    g[rng.random((rows, cols)) < 0.02] = 1  # marker pixels (rsframe.cc:816)
    dark = rng.random((rows, cols)) < 0.05
    g[dark] = rng.integers(0, 9, size=int(dark.sum()), dtype=np.uint8)  # black: 3 g^2 <= 225
    depth = rng.uniform(0.6, 2.5, size=(rows, cols))
    inl = np.column_stack([rng.uniform(-0.7, 0.7, m), rng.uniform(-0.45, 0.45, m), rng.normal(2.0, 1.0, m)]) if m else np.zeros((0, 3))
    return K, g, depth, inl


_expected = {}


def _oracle(oracle, rsdsfm, rows, cols, m, off, mode, q5):
    """the oracle's outputs, computed once per (shape, modes) / offset and shared"""
    key = (rows, cols, m, mode, q5)
    if key not in _expected:
        K, g, depth, inl = _inputs(rsdsfm, rows, cols, m)
        R, t = oracle.pose_table(np.array([0.3, -0.2, 0.1]), np.array([0.02, 0.03, -0.04]), 0.1, 0.9, rows)
        R = np.ascontiguousarray(R).reshape(rows, 9)
        gs3, c3 = oracle.back_project(np.repeat(g[:, :, None], 3, axis=2), depth, R, t, *K, mode=mode, q5_mode=q5)
        _expected[key] = dict(R=R, t=t, gs3=gs3, gs=np.ascontiguousarray(gs3[:, :, 0]), c3=c3, prev=oracle.depth_preview(inl, *K, rows, cols), fixed={})
    e = _expected[key]
    if off not in e["fixed"]:
        e["fixed"][off] = np.ascontiguousarray(oracle.interpolate_cracky(e["gs3"], off)[:, :, 0])
    return e


def _run(rsdsfm, torch, s, rows, cols, m, off, mode, q5, e, calls=1):
    dev = torch.device("cuda", 0)
    K, g, depth, inl = _inputs(rsdsfm, rows, cols, m)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_img, d_dm, d_R, d_t, d_inl = tt(g), tt(depth.T), tt(e["R"]), tt(e["t"]), tt(inl if m else np.zeros((1, 3)))
    outs = []
    for _ in range(calls):
        prev = torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
        gs, fixed = torch.full((rows, cols), 77, dtype=torch.uint8, device=dev), torch.full((rows, cols), 77, dtype=torch.uint8, device=dev)
        c3 = torch.full((rows, cols, 3), np.nan, dtype=torch.float32, device=dev)
        s.rectify_gray_frame_dev(d_inl.data_ptr(), m, d_img.data_ptr(), d_dm.data_ptr(), d_R.data_ptr(), d_t.data_ptr(), K, rows, cols, prev.data_ptr(),
                                 gs.data_ptr(), fixed.data_ptr(), c3.data_ptr(), mode=mode, q5_mode=q5, offset=off)
        s.synchronize()
        outs.append((prev.cpu().numpy(), gs.cpu().numpy(), fixed.cpu().numpy(), c3.cpu().numpy()))
    return outs


def _check(got, e, off):
    prev, gs, fixed, c3 = got
    assert np.array_equal(gs, e["gs"])
    assert np.array_equal(fixed, e["fixed"][off])
    assert np.array_equal(prev, e["prev"])
    assert np.array_equal(c3.view(np.uint32), e["c3"].view(np.uint32))


@pytest.mark.parametrize("rows,cols,m,off,mode,q5", CASES)
def test_gray_rectifier_equals_channel_0_of_the_oracle(oracle, rsdsfm, rows, cols, m, off, mode, q5):
    import torch

    e = _oracle(oracle, rsdsfm, rows, cols, m, off, mode, q5)
    if rows * cols > 64:
        assert (e["gs"] != 0).any() and not np.array_equal(e["gs"], e["fixed"][off])  # something landed, something was filled
    with rsdsfm.Solver(0) as s:
        _check(_run(rsdsfm, torch, s, rows, cols, m, off, mode, q5, e)[0], e, off)


def test_twice_on_one_context(oracle, rsdsfm):
    """the claim maps' epochs advance from call to call: the second call on a context sees the first one's words and ignores them"""
    import torch

    with rsdsfm.Solver(0) as s:
        for rows, cols, m, off in ((33, 68, 5000, 1), (33, 70, 5000, 2)):
            e = _oracle(oracle, rsdsfm, rows, cols, m, off, 0, 0)
            for got in _run(rsdsfm, torch, s, rows, cols, m, off, 0, 0, e, calls=2):
                _check(got, e, off)


def test_aliased_outputs_raise(rsdsfm):
    import torch

    dev = torch.device("cuda", 0)
    rows, cols = 16, 64
    img = torch.zeros((rows, cols), dtype=torch.uint8, device=dev)
    dm, R, t = torch.ones(rows * cols, dtype=torch.float64, device=dev), torch.zeros(rows * 9, dtype=torch.float64, device=dev), torch.zeros(rows * 3, dtype=torch.float64, device=dev)
    prev, gs = torch.zeros_like(img), torch.zeros_like(img)
    with rsdsfm.Solver(0) as s:
        with pytest.raises(rsdsfm.RsdsfmError):
            s.rectify_gray_frame_dev(0, 0, img.data_ptr(), dm.data_ptr(), R.data_ptr(), t.data_ptr(), (50.0, 50.0, 32.0, 8.0), rows, cols, prev.data_ptr(),
                                     gs.data_ptr(), gs.data_ptr())
