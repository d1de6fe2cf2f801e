"""Timing of the stabiliser's border fill at 1280x720 ("Border fill"), one process, HIP events on the context's stream,
medians over repeated, warmed-up calls:

  (a) rsdsfm_stabilize_frame_dev, the yardstick, against one rsdsfm_stabilize_fill_frame_dev (b) on a mask that is 90 % set (the band along
      two edges empty, as a stabilised frame leaves it) and (c) on an empty mask, BGR, with the source plane and the counter, on one solved
      pair of a render_sequence clip with a share --holes of its depth map zeroed at random; the three alternate, so that all see the same
      machine.  The in-out planes are restored before every timed call, outside the timed window;
  (d) rsdsfm_stabilize_video_dev against (e) rsdsfm_stabilize_video_filled_dev at radius 2 over 16 pairs at B = 8, alternating, per pair.
The expectation (stages A and B are the same and the fill-warp kernel reads less than stage C) is that (b) costs no more
than (a) measured in the same run, and that (e) - (d) is about four such passes per pair; every line says whether that held.  One JSON line
per measurement; the record is profiles/stabilize_fill_time.txt.

    python tools/stabilize_fill_time.py [--reps 20] [--clip-reps 5] [--warmup 3] [--holes 0.33] > profiles/stabilize_fill_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

RADIUS = 2


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
    # a neighbour's pose of the size a hand-held clip gives: 0.5 degrees and a hundredth of the scene's depth (tools/stabilize_time.py's)
    axis = np.array([0.005, -0.006, 0.004])
    th = np.linalg.norm(axis)
    X = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    M = np.eye(3) + np.sin(th) / th * X + (1.0 - np.cos(th)) / th ** 2 * (X @ X)
    m = np.array([0.01, -0.008, 0.004])

    def event_pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        d_a, d_b = torch.from_numpy(frames[0]).to(dev), torch.from_numpy(frames[1]).to(dev)
        flow = torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev)
        dm, R, t = (torch.zeros(n, dtype=torch.float64, device=dev) for n in (npix, ROWS * 9, ROWS * 3))
        out, mask, source = torch.empty_like(d_a), torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev), torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        filled = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        s.deep_flow_dev(d_a.data_ptr(), d_b.data_ptr(), ROWS, COLS, 3, flow.data_ptr())
        s.solve_frame_dev(flow.data_ptr(), ROWS, COLS, K, 0.8, dm.data_ptr(), R.data_ptr(), t.data_ptr(), trials=50, tol=0.05)
        s.synchronize()
        torch.manual_seed(1)
        dm.mul_((torch.rand(npix, device=dev) >= args.holes).double())  # non-inliers carry no depth
        # the starting planes: 90 % set = a band of 5.13 % of each side's length empty along the top and the left edge; and nothing set
        band_r, band_c = int(round(0.0513 * ROWS)), int(round(0.0513 * COLS))
        mask90 = torch.ones((ROWS, COLS), dtype=torch.uint8, device=dev)
        mask90[:band_r, :] = 0
        mask90[:, :band_c] = 0
        mask0 = torch.zeros_like(mask90)
        image0 = d_b.clone()
        torch.cuda.synchronize()
        common = (d_a.data_ptr(), 3, dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, ROWS, COLS)

        def restore(start):  # on the solver's stream (torch's current stream here), in front of the timed window
            if start is not None:
                out.copy_(image0), mask.copy_(start), source.copy_(start)

        fill = lambda: s.stabilize_fill_frame_dev(*common, M, m, 2, out.data_ptr(), mask.data_ptr(), source.data_ptr(), filled.data_ptr())
        calls = dict(a=(None, lambda: s.stabilize_frame_dev(*common, M, m, out.data_ptr(), mask.data_ptr())), b=(mask90, fill), c=(mask0, fill))
        for start, fn in calls.values():
            for _ in range(args.warmup):
                restore(start), fn()
        s.synchronize()
        ts, taken = dict(a=[], b=[], c=[]), {}
        for _ in range(args.reps):
            for name, (start, fn) in calls.items():
                restore(start)
                e0, e1 = event_pair()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3)
                taken[name] = int(filled.cpu())
        med = {k_: float(np.median(v_)) for k_, v_ in ts.items()}
        mm = lambda k_: [round(min(ts[k_]), 1), round(max(ts[k_]), 1)]
        print(json.dumps(dict(what="frame", size="%dx%d" % (COLS, ROWS), holes=args.holes, reps=args.reps,
                              launches=dict(a=rsdsfm.stabilize_launches(ROWS, COLS), b=rsdsfm.stabilize_fill_launches(ROWS, COLS)),
                              a_stabilize_us=round(med["a"], 1), a_min_max_us=mm("a"), b_fill_mask90_us=round(med["b"], 1), b_min_max_us=mm("b"),
                              c_fill_mask0_us=round(med["c"], 1), c_min_max_us=mm("c"), mask90_set=round(float(mask90.double().mean()), 4),
                              b_taken=taken["b"], c_taken=taken["c"], b_minus_a_us=round(med["b"] - med["a"], 1), c_minus_a_us=round(med["c"] - med["a"], 1),
                              b_no_more_than_a=bool(med["b"] <= med["a"]))), flush=True)
        # the clip: (d) and (e) alternate
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        mk = lambda shape, dt: [torch.empty(shape, dtype=dt, device=dev) for _ in range(PAIRS)]
        dms, flows, Rs, Ts = mk(npix, torch.float64), mk((ROWS, COLS, 2), torch.float64), mk(ROWS * 9, torch.float64), mk(ROWS * 3, torch.float64)
        stabs, smasks, sources = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        p = lambda xs: [x.data_ptr() for x in xs]
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        stab = lambda: s.stabilize_video_dev(p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks), trials=50, tol=0.05)
        fillv = lambda: s.stabilize_video_filled_dev(p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks), p(sources),
                                                     fill_radius=RADIUS, trials=50, tol=0.05)
        for _ in range(args.warmup):
            stab(), s.synchronize(), fillv(), s.synchronize()
        td, te = [], []
        res = None
        for _ in range(args.clip_reps):
            for fn, acc in ((stab, td), (fillv, te)):
                e0, e1 = event_pair()
                e0.record(stream)
                res = fn()
                s.synchronize()
                e1.record(stream)
                e1.synchronize()
                acc.append(e0.elapsed_time(e1) / PAIRS)
        d, e = float(np.median(td)), float(np.median(te))
        passes = sum(len(rsdsfm.neighbour_poses(res["A"], res["c"], res["A_s"], res["c_s"], res["scales"], q, RADIUS)[0]) for q in range(PAIRS)) / PAIRS
        counts = res["counts"]
        print(json.dumps(dict(what="clip", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, batch=BATCH, radius=RADIUS, reps=args.clip_reps,
                              d_stabilize_video_ms_per_pair=round(d, 3), d_min_max_ms=[round(min(td), 3), round(max(td), 3)],
                              e_filled_video_ms_per_pair=round(e, 3), e_min_max_ms=[round(min(te), 3), round(max(te), 3)],
                              e_minus_d_us_per_pair=round((e - d) * 1e3, 1), fill_passes_per_pair=round(passes, 2),
                              e_minus_d_us_per_pass=round((e - d) * 1e3 / passes, 1), e_minus_d_percent_of_d=round(100.0 * (e - d) / d, 2),
                              d_spread_percent=round(100.0 * (max(td) - min(td)) / d, 2), e_within_d_spread=bool((e - d) <= (max(td) - min(td))),
                              own_mean_share=round(float(counts[:, 1].mean()) / npix, 4), filled_mean_share=round(float(counts[:, 2:].sum(axis=1).mean()) / npix, 4),
                              none_mean_share=round(float(counts[:, 0].mean()) / npix, 4))), flush=True)


if __name__ == "__main__":
    main()
