"""Timing of the forward-backward flow check at 1280x720 ("Forward-backward flow check"), one process, HIP events on the
context's stream, medians over repeated, warmed-up calls, the variants of one comparison alternating:

  (1) rsdsfm_flow_consistency_dev alone (mask + masked field + count; with the residual; the mask alone), ten calls per event pair, against the HBM floor of the
      bytes it moves (flow_check_kernels.hip: 49 B per pixel, 57 B with the residual, at the 8.0 TB/s peak);
  (2) the checked pair against its yardstick: (a) two back-to-back rsdsfm_deep_flow_dev calls (forward, backward), (b)
      rsdsfm_deep_flow_checked_dev = two passes on the pair workspace + the check in place (the form the library has), (c) the other form,
      put together from public calls: rsdsfm_deep_flow_seq_dev over the frames {1, 2, 1} at B = 2 (one batch of two, every launch serving
      both directions) + rsdsfm_flow_consistency_dev in place; (b) and (c) must give the same bytes;
  (3) rsdsfm_solve_video_dev and rsdsfm_solve_video_checked_dev over 16 pairs at B = 8, per pair, with the spread of each one's repetitions.
The clip is a render_sequence clip with a block that moves on its own, so that the check has something to reject.
One JSON line per measurement; the record is profiles/flow_check_time.txt.

    python tools/flow_check_time.py [--reps 30] [--flow-reps 9] [--clip-reps 7] [--warmup 3] > profiles/flow_check_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS, PAIRS, BATCH = 720, 1280, 16, 8
HBM_PEAK = 8.0e12  # bytes per second


def clip(rsdsfm, nframes):
    K = (0.75 * COLS, 0.75 * COLS, 0.5 * COLS, 0.5 * ROWS)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(ROWS, COLS, K, v, w, k, 0.8, _model_only=True)
    s = 5.0 / np.abs(f0).max()
    frames, _, _ = rsdsfm.synth.render_sequence(nframes, ROWS, COLS, K, v * s, w * s, k, 0.8, seed=1)
    frames = frames.copy()
    patch = frames[0, 60:260, 900:1200][:, :, ::-1].copy()
    for j in range(nframes):  # a 200 x 300 block moving by (9, -4) pixels per frame over the background
        frames[j, 400 - 4 * j:600 - 4 * j, 300 + 9 * j:600 + 9 * j] = patch
    return frames, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--flow-reps", type=int, default=9)
    ap.add_argument("--clip-reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    frames, K = clip(rsdsfm, PAIRS + 1)
    npix = ROWS * COLS

    def once(s, fn, inner, wait):
        """ms per call of `inner` calls of fn between two events on the stream; wait: the call leaves work on other streams (the lanes)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(inner):
            fn()
        if wait:
            s.synchronize()  # (solve_video_dev returns with its lanes still running)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / inner

    def alternating(s, fns, reps, inner=1, wait=False):
        """ms of every fn, repetition by repetition in turn; per fn (median, min, max)"""
        for _ in range(args.warmup):
            for fn in fns:
                fn()
                s.synchronize()
        ts = [[] for _ in fns]
        for _ in range(reps):
            for fn, acc in zip(fns, ts):
                acc.append(once(s, fn, inner, wait))
        return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]

    with torch.cuda.device(dev), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        d_a, d_b = torch.from_numpy(frames[0]).to(dev), torch.from_numpy(frames[1]).to(dev)
        field = lambda: torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev)
        fwd, bwd, masked, work, bwd2 = field(), field(), field(), field(), field()
        mask, mask2 = (torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev) for _ in range(2))
        resid = torch.empty((ROWS, COLS), dtype=torch.float64, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        two_flows = lambda out_f, out_b: (s.deep_flow_dev(d_a.data_ptr(), d_b.data_ptr(), ROWS, COLS, 3, out_f.data_ptr()),
                                          s.deep_flow_dev(d_b.data_ptr(), d_a.data_ptr(), ROWS, COLS, 3, out_b.data_ptr()))
        two_flows(fwd, bwd)
        s.synchronize()
        # (1) the check alone
        plain = lambda: s.flow_consistency_dev(fwd.data_ptr(), bwd.data_ptr(), ROWS, COLS, mask.data_ptr(), masked.data_ptr(), None, count.data_ptr())
        with_resid = lambda: s.flow_consistency_dev(fwd.data_ptr(), bwd.data_ptr(), ROWS, COLS, mask.data_ptr(), masked.data_ptr(), resid.data_ptr(), count.data_ptr())
        mask_only = lambda: s.flow_consistency_dev(fwd.data_ptr(), bwd.data_ptr(), ROWS, COLS, mask.data_ptr())
        t = alternating(s, [plain, with_resid, mask_only], args.reps, inner=10)  # ten calls back to back per event pair: the call, not the event's latency
        consistent = int(count.cpu()[0])
        for name, bytes_px, r in (("mask + masked field + count", 49, t[0]), ("... + residual", 57, t[1]), ("mask only", 33, t[2])):
            floor_us = bytes_px * npix / HBM_PEAK * 1e6
            print(json.dumps(dict(what="check", outputs=name, size="%dx%d" % (COLS, ROWS), consistent_share=round(consistent / npix, 4), us=round(r[0] * 1e3, 1),
                                  min_max_us=[round(r[1] * 1e3, 1), round(r[2] * 1e3, 1)], bytes_per_pixel=bytes_px, hbm_floor_us=round(floor_us, 1),
                                  over_floor=round(r[0] * 1e3 / floor_us, 2))), flush=True)
        # (2) the checked pair
        simple = lambda: s.deep_flow_checked_dev(d_a.data_ptr(), d_b.data_ptr(), ROWS, COLS, 3, masked.data_ptr(), mask.data_ptr(), d_bwd=bwd.data_ptr(),
                                                 d_count=count.data_ptr())
        s.set_flow_batch(2)
        aba, out2 = [d_a.data_ptr(), d_b.data_ptr(), d_a.data_ptr()], [work.data_ptr(), bwd2.data_ptr()]
        batched = lambda: (s.deep_flow_seq_dev(aba, ROWS, COLS, 3, out2),
                           s.flow_consistency_dev(work.data_ptr(), bwd2.data_ptr(), ROWS, COLS, mask2.data_ptr(), work.data_ptr(), None, count.data_ptr()))
        simple(), batched(), s.synchronize()
        same = bool(torch.equal(mask, mask2) and torch.equal(masked.view(torch.int64), work.view(torch.int64)) and torch.equal(bwd.view(torch.int64), bwd2.view(torch.int64)))
        a, b, c = alternating(s, [lambda: two_flows(fwd, bwd2), simple, batched], args.flow_reps)
        print(json.dumps(dict(what="checked pair", size="%dx%d" % (COLS, ROWS), a_two_deep_flow_dev_ms=round(a[0], 3), a_min_max_ms=[round(a[1], 3), round(a[2], 3)],
                              b_deep_flow_checked_dev_ms=round(b[0], 3), b_min_max_ms=[round(b[1], 3), round(b[2], 3)], c_batch_of_two_plus_check_ms=round(c[0], 3),
                              c_min_max_ms=[round(c[1], 3), round(c[2], 3)], b_minus_a_us=round((b[0] - a[0]) * 1e3, 1), b_over_a=round(b[0] / a[0], 3),
                              c_over_a=round(c[0] / a[0], 3), b_and_c_same_bytes=same)), flush=True)
        # (3) the clip
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        dms = [torch.empty(npix, dtype=torch.float64, device=dev) for _ in range(PAIRS)]
        masks = [torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev) for _ in range(PAIRS)]
        fp, mp, kp = [x.data_ptr() for x in d_frames], [x.data_ptr() for x in dms], [x.data_ptr() for x in masks]
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        res = {}
        solve = lambda: res.__setitem__("plain", s.solve_video_dev(fp, ROWS, COLS, 3, K, 0.8, mp, trials=50, tol=0.05))
        checked = lambda: res.__setitem__("checked", s.solve_video_checked_dev(fp, ROWS, COLS, 3, K, 0.8, mp, kp, trials=50, tol=0.05))
        c, d = alternating(s, [solve, checked], args.clip_reps, wait=True)
        fields = [field() for _ in range(PAIRS)]
        flp = [x.data_ptr() for x in fields]
        torch.cuda.synchronize()
        flow_ms = alternating(s, [lambda: s.deep_flow_seq_dev(fp, ROWS, COLS, 3, flp)], 3)[0][0] / PAIRS  # the forward fields alone, for scale
        print(json.dumps(dict(what="clip", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, batch=BATCH, solve_video_ms_per_pair=round(c[0] / PAIRS, 3),
                              solve_video_min_max_ms=[round(c[1] / PAIRS, 3), round(c[2] / PAIRS, 3)], solve_video_spread_percent=round(100.0 * (c[2] - c[1]) / c[0], 2),
                              checked_ms_per_pair=round(d[0] / PAIRS, 3), checked_min_max_ms=[round(d[1] / PAIRS, 3), round(d[2] / PAIRS, 3)],
                              checked_spread_percent=round(100.0 * (d[2] - d[1]) / d[0], 2), checked_over_plain=round(d[0] / c[0], 3),
                              checked_minus_plain_ms_per_pair=round((d[0] - c[0]) / PAIRS, 3), flow_alone_ms_per_pair=round(flow_ms, 3),
                              consistent_share=round(float(np.mean([r["consistent"] for r in res["checked"]])) / npix, 4),
                              inliers_plain=int(np.mean([r["num_inliers"] for r in res["plain"]])), inliers_checked=int(np.mean([r["num_inliers"] for r in res["checked"]])),
                              points_checked=int(np.mean([r["n"] for r in res["checked"]])))), flush=True)


if __name__ == "__main__":
    main()
