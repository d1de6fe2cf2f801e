"""Timing of the clean plate at 1280x720 BGR ("Clean plate"), one process, HIP events on the context's stream, medians over
repeated, warmed-up calls (tools/denoise_time.py's protocol); the variants of a group alternate, so that all see the same machine:

  (a) rsdsfm_plate_median_dev at 3, 5 and 15 sources (2, 4 and 14 layers, each 90 % set and within +-5 of the reference), with the votes, the flag
      plane and the counters and without any of them, and beside them, in the same run, the FOUR rsdsfm_denoise_accumulate_dev launches that serve
      the same five sources (first, mid, mid, last with the weight plane and counters) -- the existing launches are the yardstick;
  (b) one rsdsfm_plate_frame_dev at radius 2 (frame 2 of a solved render_sequence clip with sensor noise, five sources, on the smoothed path)
      against (c) its five rsdsfm_stabilize_window_frame_dev calls alone, onto planes zeroed as the frame call zeroes them; the difference is
      what the four records and the median cost;
  (d) rsdsfm_plate_video_dev at radius 2 on the 16-pair clip solved by rsdsfm_stabilize_video_dev, per output frame, with the counts (one copy
      and one wait at the end).
The expectation from bytes only: at five sources a BGR frame's median reads 5 (3 + 1) = 20 B and writes 3 + 1 (+ 1 + 1) B per
pixel, 22 MB, plus the halo with the flag; the four accumulate launches move 16 + 24 + 24 + 20 B per pixel.  No time is gated.  Every line says
what came out.  One JSON line per measurement; the record is profiles/plate_time.txt.

    python tools/plate_time.py [--reps 20] [--clip-reps 5] [--warmup 3] > profiles/plate_time.txt
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
        # (a) the median alone, and the denoise's four launches on the same five sources
        ref = frames[0]
        d_ref, d_full = up(ref), up(np.ones((ROWS, COLS), dtype=np.uint8))
        d_layers, d_masks = [], []
        for j in range(14):
            mask_set = np.ones((ROWS, COLS), dtype=np.uint8)
            band = (j % 4 + 1) * COLS // 40  # a band along one edge, as a moved camera leaves it: 2.5 .. 10 %
            if j % 2:
                mask_set[:, :band] = 0
            else:
                mask_set[:, COLS - band:] = 0
            d_masks.append(up(mask_set))
            d_layers.append(up(np.clip(ref.astype(np.int64) + rng.integers(-5, 6, size=ref.shape), 0, 255).astype(np.uint8)))
        d_recs = torch.zeros(14 * 8, dtype=torch.int64, device=dev)
        d_rec = torch.zeros(8, dtype=torch.int64, device=dev)
        d_cells = torch.zeros((ROWS, COLS, 4), dtype=torch.int16, device=dev)
        out, mask, votes, moving, wplane = torch.empty_like(d_ref), u8(), u8(), u8(), u8()
        counts, counts3 = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ptr = lambda xs: [x.data_ptr() for x in xs]

        def median(L, extras):
            li, lm = ptr(d_layers[:L]), ptr(d_masks[:L])
            return lambda: s.plate_median_dev(d_ref.data_ptr(), d_full.data_ptr(), li, lm, 3, ROWS, COLS, out.data_ptr(), mask.data_ptr(), votes.data_ptr() if extras else None,
                                              moving.data_ptr() if extras else None, counts.data_ptr() if extras else None, d_recs.data_ptr())

        def acc(j, first, last):
            return lambda: s.denoise_accumulate_dev(d_ref.data_ptr(), d_full.data_ptr(), d_layers[j].data_ptr(), d_masks[j].data_ptr(), 3, ROWS, COLS, d_cells.data_ptr(), first,
                                                    last, d_rec.data_ptr(), 0, 0, 12, out.data_ptr(), mask.data_ptr(), wplane.data_ptr() if last else None,
                                                    counts3.data_ptr() if last else None)

        four = [acc(0, True, False), acc(1, False, False), acc(2, False, False), acc(3, False, True)]

        def four_accumulates():
            for fn in four:
                fn()

        calls = {}
        for nsrc in (3, 5, 15):
            calls["median, %d sources, votes, flag plane and counters" % nsrc] = median(nsrc - 1, True)
            calls["median, %d sources, plate and mask only" % nsrc] = median(nsrc - 1, False)
        calls["denoise: the four accumulate launches of five sources (first, mid, mid, last)"] = four_accumulates
        for i, name in enumerate(("first", "mid (1)", "mid (2)", "last, weight plane and counters")):  # in this order, so that the cells stay a five-source sum
            calls["denoise accumulate: " + name] = four[i]
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        ts = timed(calls, args.reps)
        for name in calls:
            launches = 4 if name.startswith("denoise: the four") else 1
            print(json.dumps(dict(what=name, size="%dx%d" % (COLS, ROWS), channels=3, reps=args.reps, launches=launches, us=med(ts[name]), min_max_us=mm(ts[name]))), flush=True)
        m5 = float(np.median(ts["median, 5 sources, votes, flag plane and counters"]))
        f4 = float(np.median(ts["denoise: the four accumulate launches of five sources (first, mid, mid, last)"]))
        print(json.dumps(dict(what="median at 5 sources / the four accumulate launches", ratio=round(m5 / f4, 2), median_us=round(m5, 1), four_accumulates_us=round(f4, 1),
                              bytes_per_pixel=dict(median="20 read + 6 written", accumulates="16 + 24 + 24 + 20"),
                              counts_unset_static_moving_undecided=counts.cpu().numpy().tolist())), flush=True)
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
        # (b) and (c): frame 2 at radius 2 against its five window renders
        q = 2
        _, _, M0, m0, _, _ = rsdsfm.retime_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], float(q), nsources=PAIRS)
        nb, _, Mn, mn = rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"][:PAIRS], q, RADIUS)
        src = [q] + [int(n) for n in nb]
        M, m = np.concatenate([M0, Mn]), np.concatenate([m0, mn])
        pick = lambda xs: [xs[n].data_ptr() for n in src]
        l_img, l_mask, l_src = torch.empty_like(d_frames[0]), u8(), u8()

        def plate():
            s.plate_frame_dev(pick(d_frames), 3, pick(dms), pick(Rs), pick(Ts), K, ROWS, COLS, M, m, out.data_ptr(), mask.data_ptr(), votes.data_ptr(), moving.data_ptr(),
                              counts.data_ptr())

        def five_renders():
            for k, n in enumerate(src):
                l_img.zero_()
                l_mask.zero_()
                if k == 0:
                    l_src.zero_()
                s.stabilize_window_frame_dev(d_frames[n].data_ptr(), 3, dms[n].data_ptr(), Rs[n].data_ptr(), Ts[n].data_ptr(), K, ROWS, COLS, M[k], m[k], 1 if k == 0 else 2,
                                             (0, 0, ROWS, COLS), l_img.data_ptr(), l_mask.data_ptr(), l_src.data_ptr() if k == 0 else None)

        calls = dict(b=plate, c=five_renders)
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        ts = timed(calls, args.reps)
        plate()
        s.synchronize()
        b, c = float(np.median(ts["b"])), float(np.median(ts["c"]))
        print(json.dumps(dict(what="frame %d at radius %d, %d sources" % (q, RADIUS, len(src)), size="%dx%d" % (COLS, ROWS), channels=3, reps=args.reps,
                              launches=dict(plate=rsdsfm.plate_launches(ROWS, COLS, len(src)), renders=len(src) * rsdsfm.stabilize_window_launches(ROWS, COLS)),
                              plate_frame_us=med(ts["b"]), plate_frame_min_max_us=mm(ts["b"]), five_window_renders_us=med(ts["c"]),
                              five_window_renders_min_max_us=mm(ts["c"]), plate_minus_renders_us=round(b - c, 1), renders_spread_us=round(max(ts["c"]) - min(ts["c"]), 1),
                              counts_unset_static_moving_undecided=counts.cpu().numpy().tolist(), mean_votes=round(float(votes.float().mean().item()), 2))), flush=True)
        # (d) the clip at radius 2
        outs, omasks, ovotes, omoving = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], [u8() for _ in range(PAIRS)], [u8() for _ in range(PAIRS)], [u8() for _ in range(PAIRS)]
        torch.cuda.synchronize()
        video = lambda: s.plate_video_dev(p(d_frames[:PAIRS]), ROWS, COLS, 3, K, p(dms), p(Rs), p(Ts), r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p(outs), p(omasks),
                                          p(ovotes), p(omoving), radius=RADIUS)
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
                              us_per_output_frame=med(tv), min_max_us=mm(tv), counts_sum_unset_static_moving_undecided=res["counts"].sum(axis=0).tolist())), flush=True)


if __name__ == "__main__":
    main()
