"""Timing of the spatial top-up at 1280x720 BGR ("Spatial top-up"), one process, HIP events on the context's stream, medians
of 20 repeated, warmed-up calls (tools/denoise_time.py's protocol); the variants of a group alternate, so that all see the same machine:

  (a) rsdsfm_denoise_spatial_dev at search 1, 2 and 3 with the support plane and the counters, on a frame with every pixel deficient (no weight
      plane), on the temporal stage's real weight plane (frame 2 of the solved clip at radius 2) and on a fully supported one (every weight 80:
      the early exit), at search 2 also without the support plane and the counters (no memset node), and beside them rsdsfm_denoise_accumulate_dev (a mid launch) and rsdsfm_plate_median_dev at five sources -- the existing
      launches on the same tile, the yardsticks;
  (b) one rsdsfm_denoise_spatial_frame_dev against rsdsfm_denoise_frame_dev on the same five sources;
  (c) rsdsfm_denoise_spatial_video_dev against rsdsfm_denoise_video_dev per output frame, with the counts (one copy and one wait at the end).

The expectation, stated before the run.  Bytes: the launch reads 3 + 1 + 1 and writes 3 + 1 B per pixel, 8.3 MB at this size, a few
microseconds of HBM time: the early exit should cost about what a copy launch costs, well under the accumulate's mid launch (24 B per pixel).
Elsewhere the launch is not bound by memory.  Per displacement a thread writes 4 dwords to LDS, reads 9 x 8 bytes and does four 32-bit integer
divisions (some 35 VALU instructions each) plus some 60 more: about 200 VALU wave-instructions against about 50 LDS cycles per wave, so the
VALU bounds it.  3 600 waves on 1 024 SIMDs at 4 cycles per wave-instruction and 2.4 GHz give about 1.2 us per displacement: 8, 24 and 48
displacements -> roughly 10, 28 and 56 us with every pixel deficient, plus the barriers (one per displacement); the real weight plane, which
leaves part of the workgroups on the early exit, in between.  No time is gated.  Every line says what came out, and the last says whether
the expectation held.  One JSON line per measurement; the record is profiles/denoise_spatial_time.txt.

    python tools/denoise_spatial_time.py [--reps 20] [--clip-reps 3] [--warmup 3] > profiles/denoise_spatial_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

RADIUS = 2
EXPECT_US = {1: 10.0, 2: 28.0, 3: 56.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clip-reps", type=int, default=3)
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

    med = lambda v: round(float(np.median(v)), 1)
    mm = lambda v: [round(min(v), 1), round(max(v), 1)]
    size = "%dx%d" % (COLS, ROWS)
    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        u8 = lambda: torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        p = lambda xs: [x.data_ptr() for x in xs]
        # the clip, solved once; frame 2 at radius 2 through the temporal stage gives the real weight plane
        d_frames = [up(f) for f in frames]
        mk = lambda shape, dt: [torch.empty(shape, dtype=dt, device=dev) for _ in range(PAIRS)]
        dms, flows, Rs, Ts = mk(ROWS * COLS, torch.float64), mk((ROWS, COLS, 2), torch.float64), mk(ROWS * 9, torch.float64), mk(ROWS * 3, torch.float64)
        stabs, smasks = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], mk((ROWS, COLS), torch.uint8)
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        r = s.stabilize_video_dev(p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks), trials=50, tol=0.05)
        s.synchronize()
        q = 2
        _, _, M0, m0, _, _ = rsdsfm.retime_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], float(q), nsources=PAIRS)
        nb, _, Mn, mn = rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"][:PAIRS], q, RADIUS)
        src = [q] + [int(n) for n in nb]
        M, m = np.concatenate([M0, Mn]), np.concatenate([m0, mn])
        pick = lambda xs: [xs[n].data_ptr() for n in src]
        t_img, t_mask, t_w = torch.empty_like(d_frames[0]), u8(), u8()
        out, sup = torch.empty_like(d_frames[0]), u8()
        counts3, counts6 = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(6, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def temporal():
            s.denoise_frame_dev(pick(d_frames), 3, pick(dms), pick(Rs), pick(Ts), K, ROWS, COLS, M, m, t_img.data_ptr(), t_mask.data_ptr(), t_w.data_ptr(), counts3.data_ptr())

        def both():
            s.denoise_spatial_frame_dev(pick(d_frames), 3, pick(dms), pick(Rs), pick(Ts), K, ROWS, COLS, M, m, out.data_ptr(), t_mask.data_ptr(), t_w.data_ptr(), sup.data_ptr(),
                                        counts6.data_ptr())

        temporal()
        s.synchronize()
        temporal_counts = counts3.cpu().numpy().tolist()
        # (a) the launch alone
        d_full = up(np.ones((ROWS, COLS), dtype=np.uint8))
        d_w80 = up(np.full((ROWS, COLS), 80, dtype=np.uint8))
        d_noisy = d_frames[q]

        def spatial(image, mask, weight, S, extras=True):
            return lambda: s.denoise_spatial_dev(image.data_ptr(), mask.data_ptr(), weight.data_ptr() if weight is not None else None, 3, ROWS, COLS, out.data_ptr(),
                                                 sup.data_ptr() if extras else None, counts3.data_ptr() if extras else None, 0, 0, S)

        calls = {}
        for S in (1, 2, 3):
            calls["search %d, every pixel deficient (no weight plane)" % S] = spatial(d_noisy, d_full, None, S)
            calls["search %d, the temporal stage's weight plane" % S] = spatial(t_img, t_mask, t_w, S)
            calls["search %d, fully supported (the early exit)" % S] = spatial(d_noisy, d_full, d_w80, S)
        calls["search 2, every pixel deficient, no support plane and no counters (no memset)"] = spatial(d_noisy, d_full, None, 2, False)
        calls["search 2, fully supported (the early exit), no support plane and no counters (no memset)"] = spatial(d_noisy, d_full, d_w80, 2, False)
        # the yardsticks: the accumulate's mid launch and the plate's median at five sources, on the same frames
        d_cells = torch.zeros((ROWS, COLS, 4), dtype=torch.int16, device=dev)
        d_near = up(np.clip(frames[q].astype(np.int64) + rng.integers(-5, 6, size=frames[q].shape), 0, 255).astype(np.uint8))
        p_out, p_mask = torch.empty_like(d_frames[0]), u8()
        layers = [d_frames[n] for n in (1, 3, 0, 4)]
        lmasks = [up(np.ones((ROWS, COLS), dtype=np.uint8)) for _ in range(5)]  # the calls want the reference's and every layer's planes distinct
        torch.cuda.synchronize()
        first = lambda: s.denoise_accumulate_dev(d_noisy.data_ptr(), d_full.data_ptr(), d_near.data_ptr(), lmasks[4].data_ptr(), 3, ROWS, COLS, d_cells.data_ptr(), True, False)
        calls["denoise accumulate, mid launch"] = lambda: s.denoise_accumulate_dev(d_noisy.data_ptr(), d_full.data_ptr(), d_near.data_ptr(), lmasks[4].data_ptr(), 3, ROWS,
                                                                                   COLS, d_cells.data_ptr(), False, False)
        calls["plate median, five sources"] = lambda: s.plate_median_dev(d_noisy.data_ptr(), d_full.data_ptr(), p(layers), p(lmasks[:4]), 3, ROWS, COLS, p_out.data_ptr(),
                                                                         p_mask.data_ptr())
        first()
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        ts = {k_: [] for k_ in calls}
        for _ in range(args.reps):
            first()  # a mid launch adds to the cells every time it runs: set again outside the timed span, so that n stays below 240
            for k_, v in timed(calls, 1).items():
                ts[k_] += v
        seen = {}
        for name, fn in calls.items():
            if name.startswith("search") and "no memset" not in name:
                fn()
                s.synchronize()
                seen[name] = counts3.cpu().numpy().tolist()
            print(json.dumps(dict(what=name if not name.startswith("search") else "spatial: " + name, size=size, channels=3, reps=args.reps, launches=1, us=med(ts[name]),
                                  min_max_us=mm(ts[name]), counts_unset_kept_smoothed=seen.get(name))), flush=True)
        print(json.dumps(dict(what="the temporal stage's frame %d at radius %d" % (q, RADIUS), counts_unset_own_averaged=temporal_counts,
                              mean_weight=round(float(t_w.float().mean().item()), 2))), flush=True)
        # (b) the frame call against the temporal frame call
        calls = dict(temporal=temporal, both=both)
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        tf = timed(calls, args.reps)
        print(json.dumps(dict(what="frame %d at radius %d, %d sources" % (q, RADIUS, len(src)), size=size, channels=3, reps=args.reps,
                              launches=dict(temporal=rsdsfm.denoise_launches(ROWS, COLS, len(src)), both=rsdsfm.denoise_spatial_frame_launches(ROWS, COLS, len(src))),
                              denoise_frame_us=med(tf["temporal"]), denoise_frame_min_max_us=mm(tf["temporal"]), denoise_spatial_frame_us=med(tf["both"]),
                              denoise_spatial_frame_min_max_us=mm(tf["both"]), difference_us=round(float(np.median(tf["both"])) - float(np.median(tf["temporal"])), 1),
                              counts6=counts6.cpu().numpy().tolist())), flush=True)
        # (c) the clip calls per output frame
        outs, omasks, ows, osup = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], [u8() for _ in range(PAIRS)], [u8() for _ in range(PAIRS)], [u8() for _ in range(PAIRS)]
        torch.cuda.synchronize()
        clip_args = (p(d_frames[:PAIRS]), ROWS, COLS, 3, K, p(dms), p(Rs), p(Ts), r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p(outs), p(omasks), p(ows))
        videos = dict(temporal=lambda: s.denoise_video_dev(*clip_args, radius=RADIUS), both=lambda: s.denoise_spatial_video_dev(*clip_args, p(osup), radius=RADIUS))
        tv, res = {k_: [] for k_ in videos}, {}
        for fn in videos.values():
            fn()
        for _ in range(args.clip_reps):
            for name, fn in videos.items():
                e0, e1 = event_pair()
                e0.record(stream)
                res[name] = fn()
                e1.record(stream)
                e1.synchronize()
                tv[name].append(e0.elapsed_time(e1) * 1e3 / PAIRS)
        print(json.dumps(dict(what="clip at radius %d" % RADIUS, size=size, pairs=PAIRS, output_frames=PAIRS, reps=args.clip_reps,
                              denoise_video_us_per_frame=med(tv["temporal"]), denoise_video_min_max_us=mm(tv["temporal"]), denoise_spatial_video_us_per_frame=med(tv["both"]),
                              denoise_spatial_video_min_max_us=mm(tv["both"]), counts_sum=res["both"]["counts"].sum(axis=0).tolist())), flush=True)
        # the expectation against what came out
        got = {S: float(np.median(ts["search %d, every pixel deficient (no weight plane)" % S])) for S in (1, 2, 3)}
        exit_us = float(np.median(ts["search 2, fully supported (the early exit)"]))
        mid_us = float(np.median(ts["denoise accumulate, mid launch"]))
        print(json.dumps(dict(what="expectation", expected_us_every_pixel_deficient=EXPECT_US, measured_us={S: round(v, 1) for S, v in got.items()},
                              within_a_factor_of_two=all(0.5 * EXPECT_US[S] <= got[S] <= 2.0 * EXPECT_US[S] for S in got), early_exit_us=round(exit_us, 1),
                              accumulate_mid_us=round(mid_us, 1), early_exit_below_the_accumulate=exit_us < mid_us,
                              us_per_displacement=dict(expected=1.2, measured=round((got[3] - got[1]) / 40.0, 2)),
                              fixed_us_measured=round(got[1] - 8.0 * (got[3] - got[1]) / 40.0, 1))), flush=True)


if __name__ == "__main__":
    main()
