"""GPU: DeepFlow over whole clips (include/rsdsfm_video.h) -- every pair's field bit for bit the single-pair rsdsfm_deep_flow_dev (and so
the numpy spec), at every batch size, through both entry forms and both library builds; workspace rebuilds and interleaved single-pair
calls leave the bits alone; bad arguments are rejected."""
import ctypes as C

import numpy as np
import pytest

import flow_spec_numpy as S

pytestmark = pytest.mark.gpu

NONDEFAULT = dict(fixed_point_iterations=2, sor_iterations=7, downscale=0.8)


def _clip(rsdsfm, nframes, rows, cols, seed, channels=3):
    """a render_sequence clip at a small size, motion scaled to ~2 px per pair"""
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, 0.8, _model_only=True)
    s = 2.0 / np.abs(f0).max()
    frames, _, _ = rsdsfm.synth.render_sequence(nframes, rows, cols, K, v * s, w * s, k, 0.8, seed=seed)
    return frames if channels == 3 else np.ascontiguousarray(frames[..., 1])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def solver(rsdsfm):
    with rsdsfm.Solver(0) as s:
        yield s


@pytest.mark.parametrize("rows,cols", [(37, 53), (60, 96), (120, 160)])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("params", [None, NONDEFAULT], ids=["default", "nondefault"])
def test_every_pair_is_the_single_pair_field(rsdsfm, solver, rows, cols, channels, params):
    frames = _clip(rsdsfm, 6, rows, cols, seed=rows + cols, channels=channels)
    got = solver.deep_flow_seq(frames, params)
    assert got.shape == (5, rows, cols, 2) and got.dtype == np.float64
    for p in range(5):
        want = solver.deep_flow(frames[p], frames[p + 1], params)
        assert np.array_equal(_bits(got[p]), _bits(want)), (p, np.abs(got[p] - want).max())
    assert np.abs(got).max() > 0.01


def test_three_frames_against_the_spec(rsdsfm, solver):
    frames = _clip(rsdsfm, 3, 37, 53, seed=4)
    got = solver.deep_flow_seq(frames)
    for p in range(2):
        assert np.array_equal(_bits(got[p]), _bits(S.deep_flow(frames[p], frames[p + 1]))), p


def test_batch_size_changes_no_bit(rsdsfm):
    frames = _clip(rsdsfm, 6, 60, 96, seed=8)  # 5 pairs: ragged last batches at B = 2, 3
    with rsdsfm.Solver(0) as s:
        ref = s.deep_flow_seq(frames)
        for B in (1, 2, 3, 5, 32, 0):
            s.set_flow_batch(B)
            assert np.array_equal(_bits(s.deep_flow_seq(frames)), _bits(ref)), B


def test_entry_forms_and_builds_agree(rsdsfm, solver):
    import torch

    frames = _clip(rsdsfm, 5, 120, 160, seed=5)
    ref = solver.deep_flow_seq(frames)
    dev = torch.device("cuda", 0)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    d_flows = [torch.full((120, 160, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    solver.deep_flow_seq_dev([f.data_ptr() for f in d_frames], 120, 160, 3, [f.data_ptr() for f in d_flows])
    solver.synchronize()
    for p in range(4):
        assert np.array_equal(_bits(d_flows[p].cpu().numpy()), _bits(ref[p])), p
    with rsdsfm.Solver(0, arith="fused") as sf:
        assert np.array_equal(_bits(sf.deep_flow_seq(frames)), _bits(ref))


def test_size_change_rebuilds_and_interleaving_keeps_bits(rsdsfm, solver):
    frames = _clip(rsdsfm, 4, 120, 160, seed=6)
    ref = solver.deep_flow_seq(frames)
    one = solver.deep_flow(frames[0], frames[1])
    small = solver.deep_flow_seq(frames[:, :50, :70])  # another size: the sequence workspace is rebuilt
    assert np.array_equal(_bits(small[1]), _bits(solver.deep_flow(frames[1, :50, :70], frames[2, :50, :70])))
    assert np.array_equal(_bits(solver.deep_flow_seq(frames)), _bits(ref))
    # single-pair and clip calls interleaved on one context
    for _ in range(2):
        assert np.array_equal(_bits(solver.deep_flow(frames[0], frames[1])), _bits(one))
        assert np.array_equal(_bits(solver.deep_flow_seq(frames)), _bits(ref))
    assert np.array_equal(_bits(ref[0]), _bits(one))


def test_bad_arguments_are_rejected(rsdsfm, solver):
    lib, ctx = solver.lib, solver._ctx
    INVALID = -1
    a = [np.zeros((20, 30, 3), np.uint8) for _ in range(3)]
    out = [np.zeros((20, 30, 2)) for _ in range(2)]
    fr = rsdsfm._ptr_array([x.ctypes.data for x in a])
    fl = rsdsfm._ptr_array([x.ctypes.data for x in out])
    assert lib.rsdsfm_deep_flow_seq(ctx, fr, 3, 20, 30, 3, None, fl) == 0
    assert lib.rsdsfm_deep_flow_seq(None, fr, 3, 20, 30, 3, None, fl) == INVALID
    assert lib.rsdsfm_deep_flow_seq(ctx, fr, 1, 20, 30, 3, None, fl) == INVALID  # nframes < 2
    assert lib.rsdsfm_deep_flow_seq(ctx, rsdsfm._ptr_array([a[0].ctypes.data, 0, a[2].ctypes.data]), 3, 20, 30, 3, None, fl) == INVALID
    assert lib.rsdsfm_deep_flow_seq(ctx, fr, 3, 20, 30, 3, None, rsdsfm._ptr_array([out[0].ctypes.data, 0])) == INVALID
    assert lib.rsdsfm_deep_flow_seq(ctx, None, 3, 20, 30, 3, None, fl) == INVALID
    assert lib.rsdsfm_deep_flow_seq(ctx, fr, 3, 20, 30, 2, None, fl) == INVALID  # channels
    assert lib.rsdsfm_deep_flow_seq(ctx, fr, 3, 1, 30, 3, None, fl) == INVALID  # side < 2
    assert lib.rsdsfm_deep_flow_seq(ctx, fr, 3, 20, 16385, 3, None, fl) == INVALID  # side > 16384
    assert lib.rsdsfm_deep_flow_seq_dev(ctx, None, 3, 20, 30, 3, None, None) == INVALID
    for bad in (dict(fixed_point_iterations=0), dict(downscale=1.0), dict(omega=2.0)):
        prm = rsdsfm._flow_params(bad)
        assert lib.rsdsfm_deep_flow_seq(ctx, fr, 3, 20, 30, 3, C.byref(prm), fl) == INVALID
        with pytest.raises(rsdsfm.RsdsfmError):
            solver.deep_flow_seq(np.stack(a), bad)
    for B in (-1, 33):
        assert lib.rsdsfm_set_flow_batch(ctx, B) == INVALID
    assert lib.rsdsfm_set_flow_batch(None, 4) == INVALID
    # the solve form: the same flow checks plus its own arrays (nothing runs: every call fails before a launch)
    res = (rsdsfm.FrameResult * 2)()
    prm = rsdsfm.FrameParams()
    d = C.c_double
    call = lambda frames, n, rows, ch, maps: lib.rsdsfm_solve_video_dev(ctx, frames, n, rows, 30, ch, d(20.0), d(20.0), d(15.0), d(10.0), d(0.8), None,
                                                                       C.byref(prm), None, None, maps, None, None, res)
    maps = rsdsfm._ptr_array([x.ctypes.data for x in out])
    assert call(fr, 1, 20, 3, maps) == INVALID
    assert call(fr, 3, 20, 3, rsdsfm._ptr_array([out[0].ctypes.data, 0])) == INVALID
    assert call(fr, 3, 20, 3, None) == INVALID
    assert call(fr, 3, 20, 2, maps) == INVALID
    assert call(fr, 3, 1, 3, maps) == INVALID
    assert lib.rsdsfm_solve_video_dev(ctx, fr, 3, 20, 30, 3, d(20.0), d(20.0), d(15.0), d(10.0), d(0.8), C.byref(rsdsfm._flow_params(dict(omega=0.0))),
                                      C.byref(prm), None, None, maps, None, None, res) == INVALID
