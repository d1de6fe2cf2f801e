"""Timing of the stabiliser at 1280x720 ("Stabilisation"), one process, HIP events on the context's stream, medians over
repeated, warmed-up calls:

  (a) rsdsfm_rectify_dense_frame_dev against (b) rsdsfm_stabilize_frame_dev without and (c) with the valid count, BGR, on one solved pair of a
      render_sequence clip with a share --holes of its depth map zeroed at random, alternating, so that all three see the same machine;
  (d) rsdsfm_solve_video_linked_dev against (e) rsdsfm_stabilize_video_dev over 16 pairs at B = 8, alternating, per pair -- (e) - (d) against
      the spread of (d)'s repetitions.
The expectation (a memory-bound map pass) is that (b) costs what (a) costs, (c) one small launch more, and that the clip's
per-pair cost lies inside the baseline's spread; every line says whether that held.  One JSON line per measurement; the record is
profiles/stabilize_time.txt.

    python tools/stabilize_time.py [--reps 20] [--clip-reps 5] [--warmup 3] [--holes 0.33] > profiles/stabilize_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS, PAIRS, BATCH = 720, 1280, 16, 8


def clip(rsdsfm, nframes):
    K = (0.75 * COLS, 0.75 * COLS, 0.5 * COLS, 0.5 * ROWS)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(ROWS, COLS, K, v, w, k, 0.8, _model_only=True)
    s = 5.0 / np.abs(f0).max()
    frames, _, _ = rsdsfm.synth.render_sequence(nframes, ROWS, COLS, K, v * s, w * s, k, 0.8, seed=1)
    return frames, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clip-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--holes", type=float, default=0.33, help="share of the solved depth map zeroed at random: the synthetic pair keeps every pixel")
    args = ap.parse_args()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    frames, K = clip(rsdsfm, PAIRS + 1)
    npix = ROWS * COLS
    # a virtual pose of the size a hand-held clip gives: 0.5 degrees and a hundredth of the scene's depth
    axis = np.array([0.005, -0.006, 0.004])
    th = np.linalg.norm(axis)
    X = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    M = np.eye(3) + np.sin(th) / th * X + (1.0 - np.cos(th)) / th ** 2 * (X @ X)
    m = np.array([0.01, -0.008, 0.004])

    def event_pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    with torch.cuda.device(dev), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        d_a, d_b = torch.from_numpy(frames[0]).to(dev), torch.from_numpy(frames[1]).to(dev)
        flow = torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev)
        dm, R, t = (torch.zeros(n, dtype=torch.float64, device=dev) for n in (npix, ROWS * 9, ROWS * 3))
        out, mask = torch.empty_like(d_a), torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        valid = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        s.deep_flow_dev(d_a.data_ptr(), d_b.data_ptr(), ROWS, COLS, 3, flow.data_ptr())
        s.solve_frame_dev(flow.data_ptr(), ROWS, COLS, K, 0.8, dm.data_ptr(), R.data_ptr(), t.data_ptr(), trials=50, tol=0.05)
        s.synchronize()
        torch.manual_seed(1)
        dm.mul_((torch.rand(npix, device=dev) >= args.holes).double())  # non-inliers carry no depth
        torch.cuda.synchronize()
        common = (d_a.data_ptr(), 3, dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, ROWS, COLS)
        calls = dict(a=lambda: s.rectify_dense_frame_dev(*common, out.data_ptr(), mask.data_ptr()),
                     b=lambda: s.stabilize_frame_dev(*common, M, m, out.data_ptr(), mask.data_ptr()),
                     c=lambda: s.stabilize_frame_dev(*common, M, m, out.data_ptr(), mask.data_ptr(), d_valid=valid.data_ptr()))
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        ts = dict(a=[], b=[], c=[])
        for _ in range(args.reps):
            for name, fn in calls.items():
                e0, e1 = event_pair()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3)
        med = {k_: float(np.median(v_)) for k_, v_ in ts.items()}
        spread = max(ts["a"]) - min(ts["a"])
        print(json.dumps(dict(what="frame", size="%dx%d" % (COLS, ROWS), holes=args.holes, reps=args.reps,
                              launches=dict(a=rsdsfm.rectify_dense_launches(ROWS, COLS), b=rsdsfm.stabilize_launches(ROWS, COLS), c=rsdsfm.stabilize_launches(ROWS, COLS, True)),
                              a_dense_us=round(med["a"], 1), a_min_max_us=[round(min(ts["a"]), 1), round(max(ts["a"]), 1)], b_stabilize_us=round(med["b"], 1),
                              b_min_max_us=[round(min(ts["b"]), 1), round(max(ts["b"]), 1)], c_stabilize_count_us=round(med["c"], 1),
                              c_min_max_us=[round(min(ts["c"]), 1), round(max(ts["c"]), 1)], b_minus_a_us=round(med["b"] - med["a"], 1),
                              c_minus_b_us=round(med["c"] - med["b"], 1), valid=int(valid.cpu()), covered=round(float(mask.double().mean()), 3),
                              b_within_a_spread=bool(abs(med["b"] - med["a"]) <= spread))), flush=True)
        # the clip: (d) and (e) alternate
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        mk = lambda shape, dt: [torch.empty(shape, dtype=dt, device=dev) for _ in range(PAIRS)]
        dms, flows, Rs, Ts = mk(npix, torch.float64), mk((ROWS, COLS, 2), torch.float64), mk(ROWS * 9, torch.float64), mk(ROWS * 3, torch.float64)
        stabs, smasks = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], mk((ROWS, COLS), torch.uint8)
        p = lambda xs: [x.data_ptr() for x in xs]
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        linked = lambda: s.solve_video_linked_dev(p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), d_R=p(Rs), d_t=p(Ts), trials=50, tol=0.05)
        stab = lambda: s.stabilize_video_dev(p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks), trials=50, tol=0.05)
        for _ in range(args.warmup):
            linked(), s.synchronize(), stab(), s.synchronize()
        td, te = [], []
        res = None
        for _ in range(args.clip_reps):
            for fn, acc in ((linked, td), (stab, te)):
                e0, e1 = event_pair()
                e0.record(stream)
                res = fn()
                s.synchronize()
                e1.record(stream)
                e1.synchronize()
                acc.append(e0.elapsed_time(e1) / PAIRS)
        d, e = float(np.median(td)), float(np.median(te))
        print(json.dumps(dict(what="clip", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, batch=BATCH, reps=args.clip_reps, d_linked_ms_per_pair=round(d, 3),
                              d_min_max_ms=[round(min(td), 3), round(max(td), 3)], e_stabilize_video_ms_per_pair=round(e, 3),
                              e_min_max_ms=[round(min(te), 3), round(max(te), 3)], e_minus_d_us_per_pair=round((e - d) * 1e3, 1),
                              e_minus_d_percent_of_d=round(100.0 * (e - d) / d, 2), d_spread_percent=round(100.0 * (max(td) - min(td)) / d, 2),
                              e_within_d_spread=bool((e - d) <= (max(td) - min(td))), valid_mean_share=round(float(np.mean(res["valid"])) / npix, 3))), flush=True)


if __name__ == "__main__":
    main()
