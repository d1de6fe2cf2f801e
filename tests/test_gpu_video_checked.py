"""GPU: whole clips through the checked solve (rsdsfm_solve_video_checked_dev): per pair the mask, the masked field, the backward field, the
count, the result record, the depth map and the pose tables of rsdsfm_deep_flow_checked_dev + rsdsfm_solve_frame_dev on fresh contexts -- at
every batch size and lane count, with the caller's buffers and with the library's rings; the plain clip call interleaved on the same context
returns what it returns alone; errors are numbered within the clip."""
import numpy as np
import pytest

from test_gpu_video import _buffers, _record, _scaled_motion

pytestmark = pytest.mark.gpu

TRIALS = 20


@pytest.fixture(scope="module")
def clip(rsdsfm):
    rows, cols, gamma = 120, 160, 0.8
    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = _scaled_motion(rsdsfm, rows, cols, K, gamma, 3.0)
    frames, _, _ = rsdsfm.synth.render_sequence(5, rows, cols, K, v, w, k, gamma, seed=21)
    frames = frames.copy()
    for j in range(5):  # a block that moves on its own, so that every pair has something to reject
        frames[j, 40:70, 50 + 7 * j:90 + 7 * j] = frames[0, 10:40, 100:140][:, :, ::-1]
    return frames, rows, cols, K, gamma, [3 + 5 * i for i in range(4)]


@pytest.fixture(scope="module")
def reference(rsdsfm, clip):
    """per pair, on a fresh context each: deep_flow_checked_dev, then solve_frame_dev on its output"""
    import torch

    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    want = []
    for p in range(len(frames) - 1):
        flow, bwd = (torch.empty((rows, cols, 2), dtype=torch.float64, device=dev) for _ in range(2))
        mask, count = torch.empty((rows, cols), dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
        dms, Rs, ts = _buffers(torch, dev, 1, rows, cols)
        torch.cuda.synchronize()
        with rsdsfm.Solver(0) as s:
            s.deep_flow_checked_dev(d_frames[p].data_ptr(), d_frames[p + 1].data_ptr(), rows, cols, 3, flow.data_ptr(), mask.data_ptr(), d_bwd=bwd.data_ptr(),
                                    d_count=count.data_ptr())
            r = s.solve_frame_dev(flow.data_ptr(), rows, cols, K, gamma, dms[0].data_ptr(), Rs[0].data_ptr(), ts[0].data_ptr(), trials=TRIALS, seed=seeds[p])
            s.synchronize()
        want.append(dict(record=_record(r, dms[0], Rs[0], ts[0]), mask=mask.cpu().numpy(), flow=flow.cpu().numpy(), bwd=bwd.cpu().numpy(),
                         count=int(count.cpu()[0])))
    return want


def _checked(rsdsfm, torch, s, clip, own_buffers):
    """one solve_video_checked_dev call on context s; masks start as 77 and fields as NaN"""
    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    field = lambda: [torch.full((rows, cols, 2), np.nan, dtype=torch.float64, device=dev) for _ in range(n)]
    d_flows, d_bwds = (field(), field()) if own_buffers else (None, None)
    d_masks = [torch.full((rows, cols), 77, dtype=torch.uint8, device=dev) for _ in range(n)]
    dms, Rs, ts = _buffers(torch, dev, n, rows, cols)
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a] if a is not None else None
    res = s.solve_video_checked_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(d_masks), seeds=seeds, d_flows=ptrs(d_flows),
                                    d_bwd_flows=ptrs(d_bwds), d_R=ptrs(Rs), d_t=ptrs(ts), trials=TRIALS)
    s.synchronize()
    return [dict(record=_record(r, dms[i], Rs[i], ts[i]), mask=d_masks[i].cpu().numpy(), count=r["consistent"],
                 flow=d_flows[i].cpu().numpy() if own_buffers else None, bwd=d_bwds[i].cpu().numpy() if own_buffers else None) for i, r in enumerate(res)]


def _compare(got, want):
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["mask"], w["mask"]), p
        assert g["count"] == w["count"] == int(w["mask"].sum()), p
        if g["flow"] is not None:
            assert np.array_equal(g["flow"].view(np.uint64), w["flow"].view(np.uint64)), p
            assert np.array_equal(g["bwd"].view(np.uint64), w["bwd"].view(np.uint64)), p
        assert g["record"] == w["record"], p


def test_the_clip_has_something_to_reject(clip, reference):
    rows, cols = clip[1], clip[2]
    for w in reference:
        assert 0.5 * rows * cols < w["count"] < rows * cols - 300 and w["record"][1] > 0


@pytest.mark.parametrize("batch,lanes,own_buffers", [(1, 1, True), (2, 3, True), (8, 0, True), (2, 0, False), (2, 1, False), (8, 3, False), (1, 3, False)])
def test_checked_clip_equals_the_checked_pairs(rsdsfm, clip, reference, batch, lanes, own_buffers):
    import torch

    with rsdsfm.Solver(0) as s:
        s.set_flow_batch(batch)
        s.set_sequence_lanes(lanes)
        got = _checked(rsdsfm, torch, s, clip, own_buffers)
    _compare(got, reference)


def test_plain_clip_call_interleaved_on_the_same_context(rsdsfm, clip, reference):
    """solve_video_dev before, between and after checked calls on ONE context (library rings on both sides) returns what it returns alone"""
    import torch

    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]

    def plain(s):
        dms, Rs, ts = _buffers(torch, dev, n, rows, cols)
        torch.cuda.synchronize()
        res = s.solve_video_dev([f.data_ptr() for f in d_frames], rows, cols, 3, K, gamma, [m.data_ptr() for m in dms], seeds=seeds,
                                d_R=[r.data_ptr() for r in Rs], d_t=[t.data_ptr() for t in ts], trials=TRIALS)
        s.synchronize()
        return [_record(r, dms[i], Rs[i], ts[i]) for i, r in enumerate(res)]

    with rsdsfm.Solver(0) as s:
        s.set_flow_batch(2)
        alone = plain(s)
    with rsdsfm.Solver(0) as s:
        s.set_flow_batch(2)
        first = plain(s)
        _compare(_checked(rsdsfm, torch, s, clip, False), reference)
        second = plain(s)
        _compare(_checked(rsdsfm, torch, s, clip, True), reference)
    assert first == alone and second == alone
    assert alone != [w["record"] for w in reference]  # (the check changes the solve's input: the two calls differ)


def test_errors_are_numbered_within_the_clip_and_arguments_checked(rsdsfm, clip):
    import torch

    frames, rows, cols, K, gamma, seeds = clip
    dev = torch.device("cuda", 0)
    n = len(frames) - 1
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    # pair 3 = (frame 3, frame 3): a zero field both ways, everything consistent, no point for the solve.  At B = 2 it is pair 1 of the
    # second batch (on lane 1): the message must carry its number within the clip
    d_frames[4] = d_frames[3]
    masks = [torch.zeros((rows, cols), dtype=torch.uint8, device=dev) for _ in range(n)]
    dms, _, _ = _buffers(torch, dev, n, rows, cols)
    torch.cuda.synchronize()
    ptrs = lambda a: [t.data_ptr() for t in a]
    with rsdsfm.Solver(0) as s:
        s.set_flow_batch(2)
        with pytest.raises(rsdsfm.RsdsfmError, match="pair 3: "):
            s.solve_video_checked_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), ptrs(masks), seeds=seeds, trials=TRIALS)
        s.synchronize()
        good = ptrs(masks)
        for bad_masks in (good[:2] + [0] + good[3:], good[:1] + [good[1] + 1] + good[2:]):  # a NULL mask, a misaligned mask
            with pytest.raises(rsdsfm.RsdsfmError):
                s.solve_video_checked_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), bad_masks, seeds=seeds, trials=TRIALS)
        with pytest.raises(rsdsfm.RsdsfmError):
            s.solve_video_checked_dev(ptrs(d_frames), rows, cols, 3, K, gamma, ptrs(dms), good, seeds=seeds, trials=TRIALS, a2=-1.0)
        with pytest.raises(rsdsfm.RsdsfmError):
            s.solve_video_checked_dev(ptrs(d_frames)[:1], rows, cols, 3, K, gamma, [], [], trials=TRIALS)
