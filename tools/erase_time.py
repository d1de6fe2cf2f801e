"""Timing of the mover removal at 1280x720 BGR ("Mover removal"), one process, HIP events on the context's stream, medians over
repeated, warmed-up calls (tools/plate_time.py's protocol); the variants of a group alternate, so that all see the same machine:

  (a) rsdsfm_mover_matte_dev (three launches) at the defaults (2, 2, 4) and at the largest reach (3, 8, 16) on a flag plane with one mover of
      about 5 % of the frame and a sprinkle of hot pixels' 3 x 3 blocks, beside rsdsfm_seam_distance_dev (two launches, the same kind of work)
      at feather 8 and 27 -- the matte's C -- on the flag's complement;
  (b) rsdsfm_erase_composite_dev on a frame with about 5 % matte and on an all-matte frame, with the counters, beside rsdsfm_retime_merge_dev
      on the same two images (the existing launch that also mixes two frames under masks);
  (c) one rsdsfm_erase_frame_dev at radius 2 (frame 2 of a solved render_sequence clip with sensor noise, five sources, on the smoothed path)
      beside rsdsfm_plate_frame_dev alone on the same sources; the difference is what the matte and the composite cost;
  (d) rsdsfm_erase_video_dev at radius 2 on the 16-pair clip solved by rsdsfm_stabilize_video_dev, per output frame, with the counts (one copy
      and one wait at the end).
The expectation from bytes only: the matte moves 1 + 1 B per pixel and launch, the composite 5 B in and 4 B out per pixel
away from movers -- the four launches together well under the plate's median launch, which reads 20 B per pixel at five sources.  No time is
gated.  Every line says what came out.  One JSON line per measurement; the record is profiles/erase_time.txt.

    python tools/erase_time.py [--reps 20] [--clip-reps 5] [--warmup 3] > profiles/erase_time.txt
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
    args = ap.parse_args()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    frames, K = clip(rsdsfm, PAIRS + 1)
    rng = np.random.default_rng(5)
    frames = [np.clip(f.astype(np.int64) + rng.integers(-6, 7, size=f.shape), 0, 255).astype(np.uint8) for f in frames]  # sensor noise, per frame

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

    def measure(calls, launches):
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        ts = timed(calls, args.reps)
        for name in calls:
            print(json.dumps(dict(what=name, size="%dx%d" % (COLS, ROWS), channels=3, reps=args.reps, launches=launches[name], us=med(ts[name]), min_max_us=mm(ts[name]))),
                  flush=True)
        return ts

    med = lambda v: round(float(np.median(v)), 1)
    mm = lambda v: [round(min(v), 1), round(max(v), 1)]
    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        u8 = lambda: torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        # (a) the matte beside the seam distance
        flag = np.ones((ROWS, COLS), dtype=np.uint8)
        flag[200:440, 560:750] = 2  # one mover, 240 x 190 = 4.9 % of the frame
        hot = rng.integers(1, ROWS - 1, size=200), rng.integers(1, COLS - 1, size=200)
        for y, x in zip(*hot):
            flag[y - 1:y + 2, x - 1:x + 2] = 2
        d_flag, d_hole, d_matte, d_dist = up(flag), up((flag != 2).astype(np.uint8)), u8(), u8()
        torch.cuda.synchronize()
        calls = {"matte, open 2 grow 2 feather 4 (C = 8)": lambda: s.mover_matte_dev(d_flag.data_ptr(), ROWS, COLS, d_matte.data_ptr(), 2, 2, 4),
                 "seam distance, feather 8": lambda: s.seam_distance_dev(d_hole.data_ptr(), ROWS, COLS, 8, d_dist.data_ptr()),
                 "matte, open 3 grow 8 feather 16 (C = 27)": lambda: s.mover_matte_dev(d_flag.data_ptr(), ROWS, COLS, d_matte.data_ptr(), 3, 8, 16),
                 "seam distance, feather 27": lambda: s.seam_distance_dev(d_hole.data_ptr(), ROWS, COLS, 27, d_dist.data_ptr())}
        measure(calls, {k_: 3 if k_.startswith("matte") else 2 for k_ in calls})
        s.mover_matte_dev(d_flag.data_ptr(), ROWS, COLS, d_matte.data_ptr(), 2, 2, 4)
        s.synchronize()
        part = float((d_matte != 0).float().mean().item())
        # (b) the composite beside the retimer's merge
        d_ref, d_plate, d_full = up(frames[0]), up(frames[1]), up(np.ones((ROWS, COLS), dtype=np.uint8))
        d_all = up(np.full((ROWS, COLS), 4, dtype=np.uint8))
        out, mask, source = torch.empty_like(d_ref), u8(), u8()
        counts5 = torch.zeros(5, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        comp = lambda a: lambda: s.erase_composite_dev(d_ref.data_ptr(), d_full.data_ptr(), d_plate.data_ptr(), d_full.data_ptr(), a.data_ptr(), 3, ROWS, COLS, out.data_ptr(),
                                                       mask.data_ptr(), counts5.data_ptr(), feather=4)
        calls = {"composite, %.1f %% of the frame under the matte" % (100 * part): comp(d_matte), "composite, the whole frame under the matte": comp(d_all),
                 "retime merge of the same two images, source plane and counters": lambda: s.retime_merge_dev(
                     d_ref.data_ptr(), d_full.data_ptr(), d_plate.data_ptr(), d_full.data_ptr(), 3, ROWS, COLS, 32768, out.data_ptr(), mask.data_ptr(), source.data_ptr(),
                     counts5.data_ptr())}
        measure(calls, {k_: 1 for k_ in calls})
        # the clip, solved once
        npix = ROWS * COLS
        d_frames = [up(f) for f in frames]
        mk = lambda shape, dt: [torch.empty(shape, dtype=dt, device=dev) for _ in range(PAIRS)]
        dms, flows, Rs, Ts = mk(npix, torch.float64), mk((ROWS, COLS, 2), torch.float64), mk(ROWS * 9, torch.float64), mk(ROWS * 3, torch.float64)
        stabs, smasks = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], mk((ROWS, COLS), torch.uint8)
        p = lambda xs: [x.data_ptr() for x in xs]
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        r = s.stabilize_video_dev(p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks), trials=50, tol=0.05)
        s.synchronize()
        # (c) frame 2 at radius 2 beside the plate alone
        q = 2
        _, _, M0, m0, _, _ = rsdsfm.retime_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], float(q), nsources=PAIRS)
        nb, _, Mn, mn = rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"][:PAIRS], q, RADIUS)
        src = [q] + [int(n) for n in nb]
        M, m = np.concatenate([M0, Mn]), np.concatenate([m0, mn])
        pick = lambda xs: [xs[n].data_ptr() for n in src]
        moving, matte, counts4 = u8(), u8(), torch.zeros(4, dtype=torch.int64, device=dev)
        calls = {"erase frame": lambda: s.erase_frame_dev(pick(d_frames), 3, pick(dms), pick(Rs), pick(Ts), K, ROWS, COLS, M, m, out.data_ptr(), mask.data_ptr(), matte.data_ptr(),
                                                          moving.data_ptr(), counts5.data_ptr()),
                 "plate frame alone": lambda: s.plate_frame_dev(pick(d_frames), 3, pick(dms), pick(Rs), pick(Ts), K, ROWS, COLS, M, m, out.data_ptr(), mask.data_ptr(), None,
                                                                moving.data_ptr(), counts4.data_ptr())}
        ts = measure(calls, {"erase frame": rsdsfm.erase_launches(ROWS, COLS, len(src)), "plate frame alone": rsdsfm.plate_launches(ROWS, COLS, len(src))})
        calls["erase frame"]()
        s.synchronize()
        e, b = float(np.median(ts["erase frame"])), float(np.median(ts["plate frame alone"]))
        print(json.dumps(dict(what="frame %d at radius %d, %d sources: erase minus plate" % (q, RADIUS, len(src)), erase_minus_plate_us=round(e - b, 1),
                              plate_spread_us=round(max(ts["plate frame alone"]) - min(ts["plate frame alone"]), 1),
                              counts_unset_kept_replaced_feathered_unresolved=counts5.cpu().numpy().tolist())), flush=True)
        # (d) the clip at radius 2
        outs, omasks, omattes = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], [u8() for _ in range(PAIRS)], [u8() for _ in range(PAIRS)]
        torch.cuda.synchronize()
        video = lambda: s.erase_video_dev(p(d_frames[:PAIRS]), ROWS, COLS, 3, K, p(dms), p(Rs), p(Ts), r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p(outs), p(omasks),
                                          p(omattes), None, radius=RADIUS)
        for _ in range(args.warmup):
            video()
        tv, res = [], None
        for _ in range(args.clip_reps):
            e0, e1 = event_pair()
            e0.record(stream)
            res = video()
            e1.record(stream)
            e1.synchronize()
            tv.append(e0.elapsed_time(e1) * 1e3 / PAIRS)
        print(json.dumps(dict(what="clip at radius %d" % RADIUS, size="%dx%d" % (COLS, ROWS), pairs=PAIRS, output_frames=PAIRS, reps=args.clip_reps,
                              us_per_output_frame=med(tv), min_max_us=mm(tv), counts_sum_unset_kept_replaced_feathered_unresolved=res["counts"].sum(axis=0).tolist())), flush=True)


if __name__ == "__main__":
    main()
