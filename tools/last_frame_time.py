"""Timing of the clip's last frame at 1280x720 ("Last frame"), one process, HIP events on the context's stream, medians
over repeated, warmed-up calls:

  (a) rsdsfm_advance_depth_dev on one solved pair (its DeepFlow field, its solved map and motion), on the context's plane and without a
      counter, beside (b) the same call with a caller's plane and the counter; (a) and (b) alternate, so that both see the same machine.
      Against the HBM time of the algorithmic bytes: per pixel 8 B written (the preset), 8 B + 16 B read and one 8 B atomic (the splat),
      8 B read and 8 B written (the resolve) = 56 B, at the 6.29 TB/s a float4 copy reaches;
  (c) rsdsfm_stabilize_video_inpainted_dev at radius 2 over 16 pairs at B = 8 with last_frame = 0 against (d) the same call with
      last_frame = 1, alternating, per clip, with the spread of the repetitions.
The expectation: (a) is three launches moving 52 MB, launch-bound at a few times the HBM time; (d) - (c) is about one more
frame's rendering passes plus the advance, inside or near (c)'s own spread.  Every line says what came out.  One JSON line per
measurement; the record is profiles/last_frame_time.txt.

    python tools/last_frame_time.py [--reps 20] [--clip-reps 5] [--warmup 3] > profiles/last_frame_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

RADIUS = 2
FEATHER = 16
BYTES_PER_PIXEL = 8 + (8 + 16 + 8) + (8 + 8)
HBM_TBS = 6.29  # a float4 copy on this part


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

    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        d_a, d_b = torch.from_numpy(frames[0]).to(dev), torch.from_numpy(frames[1]).to(dev)
        flow = torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev)
        dm, R, t, out = (torch.zeros(n, dtype=torch.float64, device=dev) for n in (npix, ROWS * 9, ROWS * 3, npix))
        plane, cnt = torch.zeros(npix, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        s.deep_flow_dev(d_a.data_ptr(), d_b.data_ptr(), ROWS, COLS, 3, flow.data_ptr())
        r = s.solve_frame_dev(flow.data_ptr(), ROWS, COLS, K, 0.8, dm.data_ptr(), R.data_ptr(), t.data_ptr(), trials=50, tol=0.05)
        s.synchronize()
        held = int((dm != 0).sum().cpu())
        adv = lambda p, c: (lambda: s.advance_depth_dev(flow.data_ptr(), dm.data_ptr(), r["v"], r["w"], r["k"], ROWS, COLS, K, 0.8, out.data_ptr(), False, p, c))
        calls = dict(a=adv(None, None), b=adv(plane.data_ptr(), cnt.data_ptr()))
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        ts = {k_: [] for k_ in calls}
        for _ in range(args.reps):
            for name, fn in calls.items():
                e0, e1 = event_pair()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3)
        med = {k_: float(np.median(v_)) for k_, v_ in ts.items()}
        mm = lambda k_: [round(min(ts[k_]), 1), round(max(ts[k_]), 1)]
        hbm_us = npix * BYTES_PER_PIXEL / (HBM_TBS * 1e12) * 1e6
        print(json.dumps(dict(what="advance", size="%dx%d" % (COLS, ROWS), reps=args.reps, launches=rsdsfm.advance_depth_launches(ROWS, COLS),
                              bytes_per_pixel=BYTES_PER_PIXEL, megabytes=round(npix * BYTES_PER_PIXEL / 1e6, 1), hbm_us_at_6_29_tbs=round(hbm_us, 1),
                              a_workspace_plane_us=round(med["a"], 1), a_min_max_us=mm("a"), b_caller_plane_and_count_us=round(med["b"], 1), b_min_max_us=mm("b"),
                              a_times_hbm=round(med["a"] / hbm_us, 2), a_us_per_launch=round(med["a"] / rsdsfm.advance_depth_launches(ROWS, COLS), 2),
                              depths_in=held, depths_out=int(cnt.cpu()[0]), coverage=round(int(cnt.cpu()[0]) / max(held, 1), 4))), flush=True)
        # the clip: (c) and (d) alternate
        nf = PAIRS + 1
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        mk = lambda shape, dt: [torch.empty(shape, dtype=dt, device=dev) for _ in range(nf)]
        like = lambda: [torch.empty_like(d_frames[0]) for _ in range(nf)]
        dms, flows, Rs, Ts = mk(npix, torch.float64), mk((ROWS, COLS, 2), torch.float64)[:PAIRS], mk(ROWS * 9, torch.float64), mk(ROWS * 3, torch.float64)
        stabs, smasks, sources = like(), mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        crops, cmasks, csources = like(), mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        blends, bmasks, bsources = like(), mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        inps, isources = like(), mk((ROWS, COLS), torch.uint8)
        p = lambda xs: [x.data_ptr() for x in xs]
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        head = (p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks), p(crops), p(cmasks), p(blends), p(bmasks), p(bsources),
                p(inps), p(isources))
        kw = dict(d_crop_sources=p(csources), max_empty=npix // 100, margin=1, d_sources=p(sources), fill_radius=RADIUS, trials=50, tol=0.05, blend_feather=FEATHER)
        off = lambda: s.stabilize_video_inpainted_dev(*head, last_frame=False, **kw)
        on = lambda: s.stabilize_video_inpainted_dev(*head, last_frame=True, **kw)
        for _ in range(args.warmup):
            off(), s.synchronize(), on(), s.synchronize()
        tc, td = [], []
        res = {}
        for _ in range(args.clip_reps):
            for name, fn, acc in (("c", off, tc), ("d", on, td)):
                e0, e1 = event_pair()
                e0.record(stream)
                res[name] = fn()
                s.synchronize()
                e1.record(stream)
                e1.synchronize()
                acc.append(e0.elapsed_time(e1))
        c, d = float(np.median(tc)), float(np.median(td))
        spread = max(tc) - min(tc)
        print(json.dumps(dict(what="clip", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, batch=BATCH, radius=RADIUS, feather=FEATHER, reps=args.clip_reps,
                              windows=dict(c=list(res["c"]["window"]), d=list(res["d"]["window"])), frames_rendered=dict(c=len(res["c"]["valid"]), d=len(res["d"]["valid"])),
                              c_last_frame_0_ms_per_clip=round(c, 3), c_min_max_ms=[round(min(tc), 3), round(max(tc), 3)],
                              d_last_frame_1_ms_per_clip=round(d, 3), d_min_max_ms=[round(min(td), 3), round(max(td), 3)],
                              d_minus_c_ms=round(d - c, 3), d_minus_c_percent_of_c=round(100.0 * (d - c) / c, 2), c_per_pair_ms=round(c / PAIRS, 3),
                              c_spread_ms=round(spread, 3), c_spread_percent=round(100.0 * spread / c, 2), d_within_c_spread=bool((d - c) <= spread),
                              last_frame_valid=int(res["d"]["valid"][PAIRS]), last_frame_inpainted=int(res["d"]["inpaint_counts"][PAIRS]))), flush=True)


if __name__ == "__main__":
    main()
