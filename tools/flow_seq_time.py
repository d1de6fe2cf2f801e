"""Timing of DeepFlow over whole clips (rsdsfm_deep_flow_seq_dev, DESIGN section 12 "Sequences"): a render_sequence clip of 17 frames
(16 pairs) per size; per batch size B the median wall time per pair of deep_flow_seq_dev + synchronize over the clip, next to the
single-pair rsdsfm_deep_flow_dev median measured in the same process; and solve_video_dev (flow + solve) per pair at 1280x720.
One JSON line per size and one for the solve.

    python tools/flow_seq_time.py [--reps 5] [--batches 1,2,4,8,16] [--sizes 640x480,1280x720,1920x1080]
    python tools/flow_seq_time.py --once 1280x720 --batch 8   # warm-up, then ONE batch of B pairs (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FRAMES = 17


def clip(rows, cols, nframes):
    import rsdsfm

    K = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K, v, w, k, 0.8, _model_only=True)
    s = 5.0 / np.abs(f0).max()
    frames, _, _ = rsdsfm.synth.render_sequence(nframes, rows, cols, K, v * s, w * s, k, 0.8, seed=1)
    return frames, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--sizes", default="640x480,1280x720,1920x1080")
    ap.add_argument("--once", default=None)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    sizes = [tuple(int(x) for x in s.split("x")) for s in (args.once or args.sizes).split(",")]
    with rsdsfm.Solver(0) as s:
        for cols, rows in sizes:
            nframes = args.batch + 1 if args.once else FRAMES
            frames, K = clip(rows, cols, nframes)
            d_frames = [torch.from_numpy(f).to(dev) for f in frames]
            d_flows = [torch.empty((rows, cols, 2), dtype=torch.float64, device=dev) for _ in range(nframes - 1)]
            fp, op = [f.data_ptr() for f in d_frames], [f.data_ptr() for f in d_flows]
            torch.cuda.synchronize()
            if args.once:
                s.set_flow_batch(args.batch)
                for _ in range(args.warmup):
                    s.deep_flow_seq_dev(fp, rows, cols, 3, op)
                s.synchronize()
                s.deep_flow_seq_dev(fp, rows, cols, 3, op)
                s.synchronize()
                print(json.dumps(dict(size="%dx%d" % (cols, rows), batch=args.batch, pairs=nframes - 1)))
                continue
            # the single-pair path, same process, same frames
            one = lambda: s.deep_flow_dev(fp[0], fp[1], rows, cols, 3, op[0])
            for _ in range(args.warmup):
                one()
            s.synchronize()
            ts = []
            for _ in range(3 * args.reps):
                t0 = time.perf_counter()
                one()
                s.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            rec = dict(size="%dx%d" % (cols, rows), pairs=nframes - 1, single_pair_median_ms=round(float(np.median(ts)), 3))
            for B in [int(b) for b in args.batches.split(",")]:
                s.set_flow_batch(B)
                for _ in range(args.warmup):
                    s.deep_flow_seq_dev(fp, rows, cols, 3, op)
                s.synchronize()
                tb = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    s.deep_flow_seq_dev(fp, rows, cols, 3, op)
                    s.synchronize()
                    tb.append((time.perf_counter() - t0) * 1e3 / (nframes - 1))
                med = float(np.median(tb))
                rec["B%d_ms_per_pair" % B] = round(med, 3)
                rec["B%d_vs_single" % B] = round(med / rec["single_pair_median_ms"], 3)
            s.set_flow_batch(0)
            print(json.dumps(rec), flush=True)
            if (rows, cols) == (720, 1280):  # flow + solve of the clip in one call
                dms = [torch.empty(rows * cols, dtype=torch.float64, device=dev) for _ in range(nframes - 1)]
                mp = [m.data_ptr() for m in dms]
                torch.cuda.synchronize()
                run = lambda: s.solve_video_dev(fp, rows, cols, 3, K, 0.8, mp, d_flows=op, trials=50, tol=0.05)
                for _ in range(args.warmup):
                    run()
                tv = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    run()
                    s.synchronize()
                    tv.append((time.perf_counter() - t0) * 1e3 / (nframes - 1))
                print(json.dumps(dict(size="%dx%d" % (cols, rows), pairs=nframes - 1, solve_video_ms_per_pair=round(float(np.median(tv)), 3),
                                      batch="default")), flush=True)


if __name__ == "__main__":
    main()
