"""Timing of the synthetic shutter at 1280x720 BGR ("Synthetic shutter"), one process, HIP events on the context's stream,
medians over repeated, warmed-up calls (tools/retime_time.py's protocol); the variants of a group alternate, so that all see the same machine:

  (a) rsdsfm_shutter_accumulate_dev as the first, a mid and the last launch (the last with coverage and counters, and without either) on a sample
      that is 90 % set and on an EMPTY sample, and beside them rsdsfm_retime_merge_dev without the source plane and the counters -- the existing
      launch of the same shape, the yardstick;
  (b) one rsdsfm_shutter_frame_dev at S = 8 (t = 0.5, shutter 0.5, on the smoothed path of a solved render_sequence clip) against (c) the eight
      rsdsfm_retime_frame_dev calls at the same sub-instants, alone -- the existing call is the yardstick, not the code under test; the
      difference is what the integrator costs;
  (d) rsdsfm_shutter_video_dev at factor 1 / 2 (every second input instant) with a 180 degree shutter (one input-frame interval), S = 8, on the
      16-pair clip solved by rsdsfm_stabilize_video_dev, per output frame, with the counts (one copy and one wait at the end).
The expectation from bytes only: a mid launch on a BGR frame moves 1 + 3 + 8 + 8 = 20 B per pixel, 18 MB -- a few
microseconds, bound by the launch like the merge.  No time is gated.  Every line says what came out.  One JSON line per measurement; the record
is profiles/shutter_time.txt.

    python tools/shutter_time.py [--reps 20] [--clip-reps 5] [--warmup 3] > profiles/shutter_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

SAMPLES = 8


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

    def timed(calls, reps):
        """calls: name -> function; every repetition runs each once, in turn -> name -> list of microseconds"""
        ts = {k_: [] for k_ in calls}
        for _ in range(reps):
            for name, fn in calls.items():
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
        # (a) the accumulate alone
        sample = frames[0]
        mask_set = np.ones((ROWS, COLS), dtype=np.uint8)
        mask_set[:, :COLS // 10] = 0  # a band along one edge, as a moved camera leaves it
        d_img, d_set, d_zero = up(sample), up(mask_set), up(np.zeros((ROWS, COLS), dtype=np.uint8))
        d_other = up(np.clip(sample.astype(np.int64) + 5, 0, 255).astype(np.uint8))
        d_cells = torch.zeros((ROWS, COLS, 4), dtype=torch.int16, device=dev)
        out, mask, cov = torch.empty_like(d_img), u8(), u8()
        counts = torch.zeros(3, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        acc = lambda k, first, last, extras: (lambda: s.shutter_accumulate_dev(d_img.data_ptr(), k.data_ptr(), 3, ROWS, COLS, d_cells.data_ptr(), first, last, SAMPLES, 1,
                                                                               out.data_ptr(), mask.data_ptr(), cov.data_ptr() if extras else None,
                                                                               counts.data_ptr() if extras else None))
        bare = lambda: s.retime_merge_dev(d_img.data_ptr(), d_set.data_ptr(), d_other.data_ptr(), d_set.data_ptr(), 3, ROWS, COLS, 32768, out.data_ptr(), mask.data_ptr())
        # the cells hold a first sample while the mid and last launches are timed: a mid launch adds to them every time, 26 times in all, n <= 64
        calls = {"first, 90 % set": acc(d_set, True, False, False), "first, empty": acc(d_zero, True, False, False)}
        calls2 = {"mid, 90 % set": acc(d_set, False, False, False), "mid, empty": acc(d_zero, False, False, False),
                  "last, 90 % set, coverage and counters": acc(d_set, False, True, True), "last, empty, coverage and counters": acc(d_zero, False, True, True),
                  "last, 90 % set, no coverage and no counters (no memset)": acc(d_set, False, True, False),
                  "retime merge, both layers 90 % set, no source plane and no counters": bare}
        assert args.reps + args.warmup + 2 < 64
        for group in (calls, calls2):
            for fn in group.values():
                for _ in range(args.warmup):
                    fn()
            s.synchronize()
        ts = timed(calls, args.reps)
        acc(d_set, True, False, False)()  # one sample in the cells
        s.synchronize()
        ts.update(timed(calls2, args.reps))
        for name in list(calls) + list(calls2):
            print(json.dumps(dict(what="accumulate: " + name if not name.startswith("retime") else name, size="%dx%d" % (COLS, ROWS), channels=3, reps=args.reps, launches=1,
                                  us=med(ts[name]), min_max_us=mm(ts[name]))), flush=True)
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
        solved = (p(d_frames), ROWS, COLS, 3, K, p(dms), p(Rs), p(Ts), r["A"], r["c"], r["A_s"], r["c_s"], r["scales"])
        # (b) and (c): one exposed frame at t = 0.5 against its eight retimed frames
        t0, width = 0.5, 0.5
        sub = rsdsfm.shutter_times(t0, width, SAMPLES, PAIRS)
        poses = [rsdsfm.retime_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], tj, nsources=PAIRS) for tj in sub]
        r_img, r_mask = torch.empty_like(d_frames[0]), u8()

        def exposed():
            s.shutter_frame_dev(*solved, t0, out.data_ptr(), mask.data_ptr(), cov.data_ptr(), counts.data_ptr(), shutter=width, samples=SAMPLES)

        def eight_retimed():
            for src, w, M, m, _, _ in poses:
                s.retime_frame_dev([d_frames[q].data_ptr() for q in src], 3, [dms[q].data_ptr() for q in src], [Rs[q].data_ptr() for q in src],
                                   [Ts[q].data_ptr() for q in src], K, ROWS, COLS, M, m, w, r_img.data_ptr(), r_mask.data_ptr())

        calls = dict(b=exposed, c=eight_retimed)
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        ts = timed(calls, args.reps)
        exposed()
        s.synchronize()
        n1 = sum(1 for src, *_ in poses if len(src) == 1)
        b, c = float(np.median(ts["b"])), float(np.median(ts["c"]))
        print(json.dumps(dict(what="frame at t = 0.5, shutter 0.5, S = 8", size="%dx%d" % (COLS, ROWS), channels=3, reps=args.reps, kept=len(sub),
                              launches=dict(shutter=rsdsfm.shutter_launches(ROWS, COLS, n1, len(sub) - n1),
                                            retimed=n1 * rsdsfm.retime_launches(ROWS, COLS, 1) + (len(sub) - n1) * rsdsfm.retime_launches(ROWS, COLS, 2)),
                              shutter_frame_us=med(ts["b"]), shutter_frame_min_max_us=mm(ts["b"]), eight_retime_frames_us=med(ts["c"]),
                              eight_retime_frames_min_max_us=mm(ts["c"]), shutter_minus_retimed_us=round(b - c, 1), per_sample_us=round((b - c) / len(sub), 1),
                              retimed_spread_us=round(max(ts["c"]) - min(ts["c"]), 1), counts_unset_partial_full=counts.cpu().numpy().tolist())), flush=True)
        # (d) the clip at factor 1 / 2 with a 180 degree shutter
        times = np.arange(0, PAIRS, 2, dtype=np.float64)
        width = rsdsfm.shutter_from_angle(180, 0.5)
        nt = len(times)
        outs, omasks, ocovs = [torch.empty_like(d_frames[0]) for _ in range(nt)], [u8() for _ in range(nt)], [u8() for _ in range(nt)]
        torch.cuda.synchronize()
        video = lambda: s.shutter_video_dev(*solved, times, p(outs), p(omasks), p(ocovs), shutter=width, samples=SAMPLES)
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
        print(json.dumps(dict(what="clip at factor 1/2, 180 degree shutter, S = 8", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, shutter=width, output_frames=nt,
                              reps=args.clip_reps, us_per_output_frame=med(tv), min_max_us=mm(tv), kept=res["kept"].tolist(),
                              counts_sum_unset_partial_full=res["counts"].sum(axis=0).tolist())), flush=True)


if __name__ == "__main__":
    main()
