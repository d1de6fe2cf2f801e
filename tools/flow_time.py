"""Timing of the DeepFlow front end (rsdsfm_deep_flow_dev): median wall time of one pair, device buffers in and out
(enqueue + synchronize), after a warm-up, at 640x480, 1280x720 and 1920x1080.  One JSON line per size.

    python tools/flow_time.py [--pairs 30] [--warmup 5] [--sizes 640x480,1280x720,1920x1080]
    python tools/flow_time.py --once 1280x720     # warm-up, then ONE pair (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pair(rows, cols):
    import rsdsfm

    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, 0.8, _model_only=True)
    s = 5.0 / np.abs(f0).max()
    a, b, _, _ = rsdsfm.synth.render_pair(rows, cols, K, v * s, w * s, k, 0.8, seed=1)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="640x480,1280x720,1920x1080")
    ap.add_argument("--once", default=None)
    args = ap.parse_args()
    import torch

    import rsdsfm

    sizes = [tuple(int(x) for x in s.split("x")) for s in (args.once or args.sizes).split(",")]
    dev = torch.device("cuda", 0)
    with rsdsfm.Solver(0) as s:
        for cols, rows in sizes:
            a, b = pair(rows, cols)
            da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
            df = torch.empty((rows, cols, 2), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            run = lambda: s.deep_flow_dev(da.data_ptr(), db.data_ptr(), rows, cols, 3, df.data_ptr())
            for _ in range(args.warmup):
                run()
            s.synchronize()
            if args.once:
                run()
                s.synchronize()
                print(json.dumps(dict(size="%dx%d" % (cols, rows), pairs=1)))
                continue
            ts = []
            for _ in range(args.pairs):
                t0 = time.perf_counter()
                run()
                s.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            for _ in range(args.pairs):
                run()
            s.synchronize()
            back = (time.perf_counter() - t0) * 1e3 / args.pairs
            lv = rsdsfm.flow_levels(rows, cols)
            print(json.dumps(dict(size="%dx%d" % (cols, rows), levels=len(lv), pairs=args.pairs, median_ms=round(float(np.median(ts)), 3),
                                  min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), back_to_back_ms=round(back, 3))), flush=True)


if __name__ == "__main__":
    main()
