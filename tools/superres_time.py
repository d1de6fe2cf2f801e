"""Timing of the multi-frame super-resolution at scale 2 on 1280x720 BGR sources, so on fine planes of 2560x1440 (DESIGN section 12,
"Super-resolution"), one process, HIP events on the context's stream, medians over repeated, warmed-up calls (tools/denoise_time.py's
protocol); the variants of a group alternate, so that all see the same machine:

  (a) rsdsfm_superres_accumulate_dev as the first, a mid and the last launch (the last with the weight plane and counters, and without either)
      on a layer whose proximity plane is 90 % set and whose bilinear plane agrees with the reference within +-5, on a layer that disagrees
      everywhere (every weight 0: a mid launch then touches no cell and reads no nearest plane) and on an EMPTY layer, and beside them
      rsdsfm_denoise_accumulate_dev as a mid launch on planes of the SAME size -- the existing launch of the same tile and cells, the
      yardstick -- and rsdsfm_seam_overlap_sums_dev;
  (b) one rsdsfm_superres_frame_dev at scale 2, radius 2 (frame 2 of a solved render_sequence clip with sensor noise, five sources, on the
      smoothed path) against (c) its five rsdsfm_superres_render_dev calls alone; the difference is what the records and the accumulates cost;
      and beside them five rsdsfm_stabilize_window_frame_dev calls at the source size, the existing render of a quarter of the pixels;
  (d) rsdsfm_superres_video_dev at scale 2, radius 2 on the 16-pair clip solved by rsdsfm_stabilize_video_dev, per output frame, with the
      counts (one copy and one wait at the end).
The expectation from bytes only: a mid launch on a BGR frame moves 1 + 1 + 3 + 3 + 3 + 8 + 8 = 27 B per fine pixel, about 100 MB at 2560x1440,
plus the halo; the denoise's mid launch moves 24.  No time is gated.  Every line says what came out.  One JSON line per measurement; the
record is profiles/superres_time.txt.

    python tools/superres_time.py [--reps 20] [--clip-reps 5] [--warmup 3] > profiles/superres_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

RADIUS = 2
SCALE = 2
FROWS, FCOLS = SCALE * ROWS, SCALE * COLS


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
        u8 = lambda: torch.empty((FROWS, FCOLS), dtype=torch.uint8, device=dev)
        # (a) the accumulate alone, on fine planes: the own frame magnified by pixel repetition stands in for a render
        ref = np.ascontiguousarray(frames[0].repeat(SCALE, axis=0).repeat(SCALE, axis=1))
        prox_set = rng.integers(1, 17, size=(FROWS, FCOLS)).astype(np.uint8)
        prox_set[:, :FCOLS // 10] = 0  # a band along one edge, as a moved camera leaves it
        mask_set = (prox_set != 0).astype(np.uint8)
        d_ref, d_rprox, d_lprox = up(ref), up(rng.integers(1, 17, size=(FROWS, FCOLS)).astype(np.uint8)), up(prox_set)
        d_full, d_set, d_zero = up(np.ones((FROWS, FCOLS), dtype=np.uint8)), up(mask_set), up(np.zeros((FROWS, FCOLS), dtype=np.uint8))
        near = lambda: up(np.clip(ref.astype(np.int64) + rng.integers(-5, 6, size=ref.shape), 0, 255).astype(np.uint8))
        d_rnear, d_lbil, d_lnear = near(), near(), near()
        d_far = up(ref ^ 0x80)
        d_cells = torch.zeros((FROWS, FCOLS, 4), dtype=torch.int16, device=dev)
        d_dcells = torch.zeros((FROWS, FCOLS, 4), dtype=torch.int16, device=dev)
        d_rec = torch.zeros(8, dtype=torch.int64, device=dev)
        out, mask, wplane = torch.empty_like(d_ref), u8(), u8()
        counts = torch.zeros(3, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def acc(lbil, lprox, first, last, extras):
            return lambda: s.superres_accumulate_dev(d_ref.data_ptr(), d_rnear.data_ptr(), d_rprox.data_ptr(), lbil.data_ptr(), d_lnear.data_ptr(), lprox.data_ptr(), 3, FROWS,
                                                     FCOLS, d_cells.data_ptr(), first, last, d_rec.data_ptr(), 0, 0, 12, out.data_ptr(), mask.data_ptr(),
                                                     wplane.data_ptr() if extras else None, counts.data_ptr() if extras else None)

        denoise_mid = lambda: s.denoise_accumulate_dev(d_ref.data_ptr(), d_full.data_ptr(), d_lbil.data_ptr(), d_set.data_ptr(), 3, FROWS, FCOLS, d_dcells.data_ptr(), False,
                                                       False, d_rec.data_ptr(), 0, 0, 12)
        denoise_first = lambda: s.denoise_accumulate_dev(d_ref.data_ptr(), d_full.data_ptr(), d_lbil.data_ptr(), d_set.data_ptr(), 3, FROWS, FCOLS, d_dcells.data_ptr(), True,
                                                         False, d_rec.data_ptr(), 0, 0, 12)
        sums = lambda: s.seam_overlap_sums_dev(d_ref.data_ptr(), d_full.data_ptr(), d_lbil.data_ptr(), d_lprox.data_ptr(), 3, FROWS, FCOLS, d_rec.data_ptr())
        # a mid launch adds to the cells every time it runs: the cells are set again by a first launch in front of every repetition's mid launches
        # (outside the timed span), so that n stays below 240 whatever the number of repetitions
        first = acc(d_lbil, d_lprox, True, False, False)
        calls = {"first, 90 % set, agrees": first, "first, empty": acc(d_lbil, d_zero, True, False, False)}
        calls2 = {"mid, 90 % set, agrees": acc(d_lbil, d_lprox, False, False, False), "mid, 90 % set, disagrees (every weight 0)": acc(d_far, d_lprox, False, False, False),
                  "mid, empty": acc(d_lbil, d_zero, False, False, False), "last, 90 % set, agrees, weight plane and counters": acc(d_lbil, d_lprox, False, True, True),
                  "last, empty, weight plane and counters": acc(d_lbil, d_zero, False, True, True),
                  "last, 90 % set, agrees, no weight plane and no counters (no memset)": acc(d_lbil, d_lprox, False, True, False),
                  "denoise accumulate, mid, 90 % set, same size": denoise_mid, "seam overlap sums, 90 % set": sums}
        sums()
        for group in (calls, calls2):
            for fn in group.values():
                for _ in range(min(args.warmup, 3)):
                    fn()
            first()
            denoise_first()
            s.synchronize()
        ts = timed(calls, args.reps)
        ts.update({k_: [] for k_ in calls2})
        for _ in range(args.reps):
            first()
            denoise_first()
            for k_, v in timed(calls2, 1).items():
                ts[k_] += v
        for name in list(calls) + list(calls2):
            what = name if name.startswith(("denoise", "seam")) else "accumulate: " + name
            print(json.dumps(dict(what=what, size="%dx%d" % (FCOLS, FROWS), channels=3, reps=args.reps, launches=1, us=med(ts[name]), min_max_us=mm(ts[name]))), flush=True)
        a_mid, d_mid = float(np.median(ts["mid, 90 % set, agrees"])), float(np.median(ts["denoise accumulate, mid, 90 % set, same size"]))
        print(json.dumps(dict(what="accumulate mid / denoise accumulate mid", ratio=round(a_mid / d_mid, 2), bytes_per_pixel=dict(superres=27, denoise=24),
                              mid_gb_per_s_at_27_bytes=round(27.0 * 0.9 * FROWS * FCOLS / a_mid / 1e3, 1))), flush=True)
        del d_far, d_dcells, d_cells, d_full, d_set, d_zero
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
        # (b) and (c): frame 2 at scale 2, radius 2 against its five renders
        q = 2
        _, _, M0, m0, _, _ = rsdsfm.retime_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], float(q), nsources=PAIRS)
        nb, _, Mn, mn = rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"][:PAIRS], q, RADIUS)
        src = [q] + [int(n) for n in nb]
        M, m = np.concatenate([M0, Mn]), np.concatenate([m0, mn])
        pick = lambda xs: [xs[n].data_ptr() for n in src]
        l_bil, l_near, l_prox = torch.empty_like(d_ref), torch.empty_like(d_ref), u8()
        c_img, c_mask = torch.empty_like(d_frames[0]), torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)

        def merged():
            s.superres_frame_dev(pick(d_frames), 3, pick(dms), pick(Rs), pick(Ts), K, ROWS, COLS, M, m, out.data_ptr(), mask.data_ptr(), wplane.data_ptr(), counts.data_ptr(),
                                 scale=SCALE)

        def five_renders():
            for k, n in enumerate(src):
                s.superres_render_dev(d_frames[n].data_ptr(), 3, dms[n].data_ptr(), Rs[n].data_ptr(), Ts[n].data_ptr(), K, ROWS, COLS, M[k], m[k], SCALE, l_bil.data_ptr(),
                                      l_near.data_ptr(), l_prox.data_ptr(), mask.data_ptr() if k == 0 else None)

        def five_coarse_renders():
            for k, n in enumerate(src):
                c_img.zero_()
                c_mask.zero_()
                s.stabilize_window_frame_dev(d_frames[n].data_ptr(), 3, dms[n].data_ptr(), Rs[n].data_ptr(), Ts[n].data_ptr(), K, ROWS, COLS, M[k], m[k], 1 if k == 0 else 2,
                                             (0, 0, ROWS, COLS), c_img.data_ptr(), c_mask.data_ptr())

        calls = dict(b=merged, c=five_renders, coarse=five_coarse_renders)
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        ts = timed(calls, args.reps)
        merged()
        s.synchronize()
        b, c = float(np.median(ts["b"])), float(np.median(ts["c"]))
        print(json.dumps(dict(what="frame %d at scale %d, radius %d, %d sources" % (q, SCALE, RADIUS, len(src)), source_size="%dx%d" % (COLS, ROWS),
                              size="%dx%d" % (FCOLS, FROWS), channels=3, reps=args.reps,
                              launches=dict(superres=rsdsfm.superres_launches(ROWS, COLS, SCALE, len(src)), renders=len(src) * rsdsfm.superres_render_launches(ROWS, COLS, SCALE)),
                              superres_frame_us=med(ts["b"]), superres_frame_min_max_us=mm(ts["b"]), five_fine_renders_us=med(ts["c"]), five_fine_renders_min_max_us=mm(ts["c"]),
                              five_window_renders_at_source_size_us=med(ts["coarse"]), five_window_renders_at_source_size_min_max_us=mm(ts["coarse"]),
                              superres_minus_renders_us=round(b - c, 1), per_neighbour_us=round((b - c) / (len(src) - 1), 1),
                              renders_spread_us=round(max(ts["c"]) - min(ts["c"]), 1), counts_unset_own_merged=counts.cpu().numpy().tolist(),
                              mean_weight=round(float(wplane.float().mean().item()), 2))), flush=True)
        # (d) the clip at scale 2, radius 2
        outs, omasks = [torch.empty_like(d_ref) for _ in range(PAIRS)], [u8() for _ in range(PAIRS)]
        torch.cuda.synchronize()
        video = lambda: s.superres_video_dev(p(d_frames[:PAIRS]), ROWS, COLS, 3, K, p(dms), p(Rs), p(Ts), r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p(outs), p(omasks),
                                             None, scale=SCALE, radius=RADIUS)
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
        print(json.dumps(dict(what="clip at scale %d, radius %d" % (SCALE, RADIUS), source_size="%dx%d" % (COLS, ROWS), size="%dx%d" % (FCOLS, FROWS), pairs=PAIRS,
                              output_frames=PAIRS, reps=args.clip_reps, us_per_output_frame=med(tv), min_max_us=mm(tv),
                              counts_sum_unset_own_merged=res["counts"].sum(axis=0).tolist())), flush=True)


if __name__ == "__main__":
    main()
