"""Timing of the retimer at 1280x720 BGR ("Retime"), one process, HIP events on the context's stream, medians over repeated,
warmed-up calls (tools/stabilize_search_time.py's protocol); the variants of a group alternate, so that all see the same machine:

  (a) rsdsfm_retime_merge_dev, with the source plane and the counters, on two layers that are both 90 % set (bands along opposite edges empty,
      layer b = layer a plus noise of +-30, so that pixels dissolve and conflict), (b) on layer a and an EMPTY layer b, (c) on two empty layers;
  (d) one rsdsfm_retime_frame_dev with two sources (frames 0 and 1 of a solved render_sequence clip at t = 0.5 on the smoothed path) against
      (e) the two rsdsfm_stabilize_window_frame_dev calls it makes, alone, onto planes zeroed outside the timed window -- the parent commit's
      call is the yardstick, not the code under test;
  (f) rsdsfm_retime_video_dev at factor 2 on the 16-pair clip solved by rsdsfm_stabilize_video_dev, per output frame, with the counts (one
      copy and one wait at the end).
The expectation from bytes only: BGR with the source plane moves 8 B in and 5 B out per pixel, 12 MB per frame -- a few
microseconds, bound by the launch.  No time is gated.  Every line says what came out.  One JSON line per measurement; the record is
profiles/retime_time.txt.

    python tools/retime_time.py [--reps 20] [--clip-reps 5] [--warmup 3] > profiles/retime_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

FACTOR = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clip-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    frames, K = clip(rsdsfm, PAIRS + 1)
    npix = ROWS * COLS

    def event_pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(calls, reps, before=None):
        """calls: name -> function; every repetition runs each once, in turn -> name -> list of microseconds"""
        ts = {k_: [] for k_ in calls}
        for _ in range(reps):
            for name, fn in calls.items():
                if before:
                    before(name)
                e0, e1 = event_pair()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3)
        return ts

    med = lambda v: round(float(np.median(v)), 1)
    mm = lambda v: [round(min(v), 1), round(max(v), 1)]
    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        u8 = lambda: torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        # (a) - (c): the merge alone
        rng = np.random.default_rng(1)
        layer_a = frames[0]
        layer_b = np.clip(layer_a.astype(np.int64) + rng.integers(-30, 31, size=layer_a.shape), 0, 255).astype(np.uint8)
        mask_a, mask_b = np.ones((ROWS, COLS), dtype=np.uint8), np.ones((ROWS, COLS), dtype=np.uint8)
        mask_a[:, :COLS // 10] = 0  # bands along opposite edges, as two neighbouring frames leave them
        mask_b[:, COLS - COLS // 10:] = 0
        d_la, d_lb, d_ma, d_mb, d_zero = up(layer_a), up(layer_b), up(mask_a), up(mask_b), up(np.zeros((ROWS, COLS), dtype=np.uint8))
        out, mask, source = torch.empty_like(d_la), u8(), u8()
        counts = torch.zeros(5, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        merge = lambda ka, kb: (lambda: s.retime_merge_dev(d_la.data_ptr(), ka.data_ptr(), d_lb.data_ptr(), kb.data_ptr(), 3, ROWS, COLS, 32768, out.data_ptr(),
                                                           mask.data_ptr(), source.data_ptr(), counts.data_ptr()))
        bare = lambda: s.retime_merge_dev(d_la.data_ptr(), d_ma.data_ptr(), d_lb.data_ptr(), d_mb.data_ptr(), 3, ROWS, COLS, 32768, out.data_ptr(), mask.data_ptr())
        calls = dict(a=merge(d_ma, d_mb), b=merge(d_ma, d_zero), c=merge(d_zero, d_zero), n=bare)
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        got = {}
        for name, fn in calls.items():
            fn()
            s.synchronize()
            got[name] = counts.cpu().numpy().tolist() if name != "n" else None  # (n passes no counters)
        ts = timed(calls, args.reps)
        for name, what in (("a", "merge, both layers 90 % set"), ("b", "merge, layer b empty"), ("c", "merge, both layers empty"),
                           ("n", "merge, both layers 90 % set, no source plane and no counters (no memset)")):
            print(json.dumps(dict(what=what, size="%dx%d" % (COLS, ROWS), channels=3, reps=args.reps, launches=rsdsfm.retime_merge_launches(), us=med(ts[name]),
                                  min_max_us=mm(ts[name]), counts_none_a_b_dissolved_conflict=got[name])), flush=True)
        # the clip, solved once
        d_frames = [up(f) for f in frames]
        mk = lambda shape, dt: [torch.empty(shape, dtype=dt, device=dev) for _ in range(PAIRS)]
        dms, flows, Rs, Ts = mk(npix, torch.float64), mk((ROWS, COLS, 2), torch.float64), mk(ROWS * 9, torch.float64), mk(ROWS * 3, torch.float64)
        stabs, smasks = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], mk((ROWS, COLS), torch.uint8)
        p = lambda xs: [x.data_ptr() for x in xs]
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        r = s.stabilize_video_dev(p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks), trials=50, tol=0.05)
        s.synchronize()
        # (d) and (e): one frame at t = 0.5
        src, w, M, m, _, _ = rsdsfm.retime_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], 0.5, nsources=PAIRS)
        l_img, l_mask = [torch.empty_like(d_frames[0]) for _ in src], [u8() for _ in src]
        full = (0, 0, ROWS, COLS)

        def frame():
            s.retime_frame_dev([d_frames[q].data_ptr() for q in src], 3, [dms[q].data_ptr() for q in src], [Rs[q].data_ptr() for q in src],
                               [Ts[q].data_ptr() for q in src], K, ROWS, COLS, M, m, w, out.data_ptr(), mask.data_ptr(), source.data_ptr(), counts.data_ptr())

        def two_windows():
            for k_, q in enumerate(src):
                s.stabilize_window_frame_dev(d_frames[q].data_ptr(), 3, dms[q].data_ptr(), Rs[q].data_ptr(), Ts[q].data_ptr(), K, ROWS, COLS, M[k_], m[k_], 1 + k_, full,
                                             l_img[k_].data_ptr(), l_mask[k_].data_ptr())

        def before(name):  # on the solver's stream (torch's current stream here), in front of the timed window
            if name == "e":
                for a in l_img + l_mask:
                    a.zero_()

        calls = dict(d=frame, e=two_windows)
        for name, fn in calls.items():
            for _ in range(args.warmup):
                before(name), fn()
        s.synchronize()
        ts = timed(calls, args.reps, before)
        frame()
        s.synchronize()
        d, e = float(np.median(ts["d"])), float(np.median(ts["e"]))
        print(json.dumps(dict(what="frame at t = 0.5, two sources", size="%dx%d" % (COLS, ROWS), channels=3, reps=args.reps,
                              launches=dict(retime=rsdsfm.retime_launches(ROWS, COLS, 2), two_windows=2 * rsdsfm.stabilize_window_launches(ROWS, COLS)),
                              retime_frame_us=med(ts["d"]), retime_frame_min_max_us=mm(ts["d"]), two_window_calls_us=med(ts["e"]), two_window_calls_min_max_us=mm(ts["e"]),
                              retime_minus_two_windows_us=round(d - e, 1), two_windows_spread_us=round(max(ts["e"]) - min(ts["e"]), 1), weight_q16=w,
                              counts_none_a_b_dissolved_conflict=counts.cpu().numpy().tolist())), flush=True)
        # (f) the clip at factor 2
        times = rsdsfm.retime_times(PAIRS, FACTOR)
        nt = len(times)
        outs, omasks, osrcs = [torch.empty_like(d_frames[0]) for _ in range(nt)], [u8() for _ in range(nt)], [u8() for _ in range(nt)]
        torch.cuda.synchronize()
        video = lambda: s.retime_video_dev(p(d_frames), ROWS, COLS, 3, K, p(dms), p(Rs), p(Ts), r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], times, p(outs), p(omasks),
                                           p(osrcs))
        for _ in range(args.warmup):
            video()
        tv, res = [], None
        for _ in range(args.clip_reps):
            e0, e1 = event_pair()
            e0.record(stream)
            res = video()
            e1.record(stream)
            e1.synchronize()
            tv.append(e0.elapsed_time(e1) * 1e3 / nt)
        print(json.dumps(dict(what="clip at factor 2", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, factor=FACTOR, output_frames=nt, reps=args.clip_reps,
                              us_per_output_frame=med(tv), min_max_us=mm(tv), two_source_frames=int((res["weights"] > 0).sum()),
                              counts_sum_none_a_b_dissolved_conflict=res["counts"].sum(axis=0).tolist())), flush=True)


if __name__ == "__main__":
    main()
