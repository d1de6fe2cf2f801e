"""Timing of the clip rectifier (rsdsfm_rectify_video_dev, DESIGN section 12 "Sequences") against the call it extends: a 17-frame
render_sequence clip (16 pairs) at 1280x720, B = 8.  In ONE run, repetition by repetition in turn: solve_video_dev (flow + solve: the
baseline), rectify_video_dev on the BGR clip, rectify_video_dev on its gray version -- wall time of the call + synchronize divided by
the pairs.  Prints one JSON line: the three medians, the spread (min, max) of the baseline's repetitions, and whether each rectifier
median lies inside that spread.

    python tools/rectify_video_time.py [--reps 9] [--warmup 2] [--size 1280x720] [--batch 8] > profiles/rectify_video_time.txt
    python tools/rectify_video_time.py --once 3   # warm-up, then ONE rectify_video_dev of the clip with 3 (or 1) channels (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_seq_time import FRAMES, clip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", default="1280x720")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--once", type=int, default=0, choices=(0, 1, 3))
    args = ap.parse_args()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    cols, rows = (int(x) for x in args.size.split("x"))
    frames, K = clip(rows, cols, FRAMES)
    # the flow's own integer BGR -> gray conversion (camera.cc:258-259): the gray clip has the BGR clip's fields and solves
    b, g, r = (frames[..., i].astype(np.int32) for i in range(3))
    gray = ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)
    n = FRAMES - 1
    ptrs = lambda ts: [t.data_ptr() for t in ts]
    mk = lambda shape, dtype: [torch.empty(shape, dtype=dtype, device=dev) for _ in range(n)]
    d_bgr, d_gray = [torch.from_numpy(f).to(dev) for f in frames], [torch.from_numpy(f).to(dev) for f in gray]
    flows, dms, prevs, c3s = mk((rows, cols, 2), torch.float64), mk((rows * cols,), torch.float64), mk((rows, cols), torch.uint8), mk((rows, cols, 3), torch.float32)
    gs3, fx3, gs1, fx1 = mk((rows, cols, 3), torch.uint8), mk((rows, cols, 3), torch.uint8), mk((rows, cols), torch.uint8), mk((rows, cols), torch.uint8)
    torch.cuda.synchronize()
    with rsdsfm.Solver(0) as s:
        s.set_flow_batch(args.batch)
        runs = dict(
            solve_video=lambda: s.solve_video_dev(ptrs(d_bgr), rows, cols, 3, K, 0.8, ptrs(dms), d_flows=ptrs(flows), trials=50, tol=0.05),
            rectify_video_bgr=lambda: s.rectify_video_dev(ptrs(d_bgr), rows, cols, 3, K, 0.8, ptrs(dms), ptrs(prevs), ptrs(gs3), ptrs(fx3), d_coords=ptrs(c3s),
                                                          d_flows=ptrs(flows), trials=50, tol=0.05),
            rectify_video_gray=lambda: s.rectify_video_dev(ptrs(d_gray), rows, cols, 1, K, 0.8, ptrs(dms), ptrs(prevs), ptrs(gs1), ptrs(fx1), d_coords=ptrs(c3s),
                                                           d_flows=ptrs(flows), trials=50, tol=0.05))
        if args.once:
            run = runs["rectify_video_bgr" if args.once == 3 else "rectify_video_gray"]
            for _ in range(args.warmup):
                run()
            s.synchronize()
            run()
            s.synchronize()
            print(json.dumps(dict(size=args.size, batch=args.batch, pairs=n, channels=args.once)))
            return
        for _ in range(args.warmup):
            for run in runs.values():
                run()
        s.synchronize()
        ts = {name: [] for name in runs}
        for _ in range(args.reps):
            for name, run in runs.items():
                t0 = time.perf_counter()
                run()
                s.synchronize()
                ts[name].append((time.perf_counter() - t0) * 1e3 / n)
    med = {name: float(np.median(v)) for name, v in ts.items()}
    lo, hi = min(ts["solve_video"]), max(ts["solve_video"])
    rec = dict(size=args.size, pairs=n, batch=args.batch, reps=args.reps, solve_video_ms_per_pair=round(med["solve_video"], 3),
               solve_video_min_ms_per_pair=round(lo, 3), solve_video_max_ms_per_pair=round(hi, 3))
    for name in ("rectify_video_bgr", "rectify_video_gray"):
        rec[name + "_ms_per_pair"] = round(med[name], 3)
        rec[name + "_vs_solve_video"] = round(med[name] / med["solve_video"], 4)
        rec[name + "_inside_solve_video_spread"] = bool(lo <= med[name] <= hi)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
