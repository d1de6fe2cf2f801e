"""Timing of the sharpness transfer at 1280x720 BGR ("Sharpness transfer"), one process, HIP events on the context's stream,
medians over repeated, warmed-up calls (tools/erase_time.py's protocol); the variants of a group alternate, so that all see the same machine:

  (a) rsdsfm_deblur_sharpness_dev beside rsdsfm_seam_overlap_sums_dev on the same reference and layer (90 % of the layer set): both read the two
      images and masks once and end in a few 64-bit atomics per workgroup;
  (b) rsdsfm_deblur_accumulate_dev as a mid launch with tau = 16, as a mid launch with tau = 0 (it returns behind the record), as the first and as
      the last launch (the last with the weight plane and the counters), beside rsdsfm_denoise_accumulate_dev in the same four places on the same
      planes -- the existing launch of the same structure, the yardstick;
  (c) one rsdsfm_deblur_frame_dev at radius 2 (frame 2 of a solved render_sequence clip with sensor noise and that frame box-blurred over 5
      columns, five sources, on the smoothed path) beside its five rsdsfm_stabilize_window_frame_dev calls alone, onto planes zeroed as the frame
      call zeroes them; the difference is what the three launches per neighbour cost;
  (d) rsdsfm_deblur_video_dev at radius 2 on the 16-pair clip solved by rsdsfm_stabilize_video_dev, per output frame, with the counts and the taus
      (one copy and one wait at the end).
The expectation to confirm or refute: both kernels are bound by their launch at this size, as the denoise's and the erase's are.  No time is gated.
Every line says what came out.  One JSON line per measurement; the record is profiles/deblur_time.txt.

    python tools/deblur_time.py [--reps 20] [--clip-reps 5] [--warmup 3] > profiles/deblur_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

RADIUS = 2
BLUR = 5
BLURRED = 2  # the clip's blurred frame


def box_blur(frame, width):
    """synth.render_sequence's blur of one frame: the rounded box mean over `width` columns, edges replicated"""
    a = frame.astype(np.int64)
    idx = np.clip(np.arange(-(width // 2), a.shape[1] + width // 2), 0, a.shape[1] - 1)
    p = a[:, idx]
    return ((2 * sum(p[:, d:d + a.shape[1]] for d in range(width)) + width) // (2 * width)).astype(np.uint8)


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
    frames = [box_blur(f, BLUR) if j == BLURRED else f for j, f in enumerate(frames)]  # the blur before the noise
    frames = [np.clip(f.astype(np.int64) + rng.integers(-6, 7, size=f.shape), 0, 255).astype(np.uint8) for f in frames]  # sensor noise, per frame
    npix = ROWS * COLS

    def event_pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(calls, reps, before=None):
        """calls: name -> function; every repetition runs `before` (untimed), then each call once, in turn -> name -> list of microseconds"""
        ts = {k_: [] for k_ in calls}
        for _ in range(reps):
            if before:
                before()
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

    def report(ts, launches=1):
        for name, v in ts.items():
            print(json.dumps(dict(what=name, size="%dx%d" % (COLS, ROWS), channels=3, reps=len(v), launches=launches, us=med(v), min_max_us=mm(v))), flush=True)

    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        u8 = lambda: torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        # (a) the sharpness launch beside the overlap sums
        sharp_frame = frames[0]
        ref = box_blur(sharp_frame, BLUR)
        mask_set = np.ones((ROWS, COLS), dtype=np.uint8)
        mask_set[:, :COLS // 10] = 0  # a band along one edge, as a moved camera leaves it
        d_ref, d_full, d_set = up(ref), up(np.ones((ROWS, COLS), dtype=np.uint8)), up(mask_set)
        d_near = up(np.clip(sharp_frame.astype(np.int64) + rng.integers(-5, 6, size=ref.shape), 0, 255).astype(np.uint8))
        d_cells = torch.zeros((ROWS, COLS, 4), dtype=torch.int16, device=dev)
        d_rec, d_T = torch.zeros(8, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
        up64 = lambda words: torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64)).to(dev)
        d_T16, d_T0 = up64([5000, 1000, 2000, 0]), up64([5000, 1000, 1000, 0])  # tau = 16 and tau = 0
        out, mask, wplane = torch.empty_like(d_ref), u8(), u8()
        counts = torch.zeros(3, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        sums = lambda: s.seam_overlap_sums_dev(d_ref.data_ptr(), d_full.data_ptr(), d_near.data_ptr(), d_set.data_ptr(), 3, ROWS, COLS, d_rec.data_ptr())
        sharpness = lambda: s.deblur_sharpness_dev(d_ref.data_ptr(), d_full.data_ptr(), d_near.data_ptr(), d_set.data_ptr(), 3, ROWS, COLS, d_T.data_ptr(), d_rec.data_ptr())
        calls = {"sharpness, 90 % set": sharpness, "seam overlap sums, 90 % set": sums}
        sums()
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        report(timed(calls, args.reps))
        T = d_T.cpu().numpy().view(np.uint64)
        print(json.dumps(dict(what="the record of (a)", pairs_AR_AL=T[:3].tolist(), tau=rsdsfm.deblur_tau(T))), flush=True)

        # (b) the accumulate beside the denoise's
        def deblur(first, last, extras, d_sharp):
            return lambda: s.deblur_accumulate_dev(d_ref.data_ptr(), d_full.data_ptr(), d_near.data_ptr(), d_set.data_ptr(), 3, ROWS, COLS, d_cells.data_ptr(), first, last,
                                                   d_sharp.data_ptr(), d_rec.data_ptr(), d_image_out=out.data_ptr(), d_mask_out=mask.data_ptr(),
                                                   d_weight=wplane.data_ptr() if extras else None, d_counts3=counts.data_ptr() if extras else None)

        def denoise(first, last, extras):
            return lambda: s.denoise_accumulate_dev(d_ref.data_ptr(), d_full.data_ptr(), d_near.data_ptr(), d_set.data_ptr(), 3, ROWS, COLS, d_cells.data_ptr(), first, last,
                                                    d_rec.data_ptr(), 0, 0, 24, out.data_ptr(), mask.data_ptr(), wplane.data_ptr() if extras else None,
                                                    counts.data_ptr() if extras else None)

        # a mid launch adds to the cells every time it runs: a first launch (untimed) sets them again in front of every repetition
        first = deblur(True, False, False, d_T16)
        calls = {"deblur accumulate: first, tau 16": first, "denoise accumulate: first": denoise(True, False, False),
                 "deblur accumulate: mid, tau 16": deblur(False, False, False, d_T16), "denoise accumulate: mid": denoise(False, False, False),
                 "deblur accumulate: mid, tau 0 (returns behind the record)": deblur(False, False, False, d_T0),
                 "deblur accumulate: last, tau 16, weight plane and counters": deblur(False, True, True, d_T16),
                 "denoise accumulate: last, weight plane and counters": denoise(False, True, True),
                 "deblur accumulate: last, tau 0, weight plane and counters": deblur(False, True, True, d_T0)}
        for fn in calls.values():
            first()
            for _ in range(min(args.warmup, 3)):
                fn()
        s.synchronize()
        report(timed(calls, args.reps, before=first))
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
        # (c) the blurred frame at radius 2 against its five window renders
        q = BLURRED
        _, _, M0, m0, _, _ = rsdsfm.retime_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], float(q), nsources=PAIRS)
        nb, _, Mn, mn = rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"][:PAIRS], q, RADIUS)
        src = [q] + [int(n) for n in nb]
        M, m = np.concatenate([M0, Mn]), np.concatenate([m0, mn])
        pick = lambda xs: [xs[n].data_ptr() for n in src]
        l_img, l_mask, l_src = torch.empty_like(d_frames[0]), u8(), u8()
        d_records = torch.zeros((len(src) - 1, 4), dtype=torch.int64, device=dev)

        def deblurred():
            s.deblur_frame_dev(pick(d_frames), 3, pick(dms), pick(Rs), pick(Ts), K, ROWS, COLS, M, m, out.data_ptr(), mask.data_ptr(), wplane.data_ptr(), counts.data_ptr(),
                               d_records.data_ptr())

        def five_renders():
            for k, n in enumerate(src):
                l_img.zero_()
                l_mask.zero_()
                if k == 0:
                    l_src.zero_()
                s.stabilize_window_frame_dev(d_frames[n].data_ptr(), 3, dms[n].data_ptr(), Rs[n].data_ptr(), Ts[n].data_ptr(), K, ROWS, COLS, M[k], m[k], 1 if k == 0 else 2,
                                             (0, 0, ROWS, COLS), l_img.data_ptr(), l_mask.data_ptr(), l_src.data_ptr() if k == 0 else None)

        calls = dict(b=deblurred, c=five_renders)
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        ts = timed(calls, args.reps)
        deblurred()
        s.synchronize()
        b, c = float(np.median(ts["b"])), float(np.median(ts["c"]))
        taus = [rsdsfm.deblur_tau(T) for T in d_records.cpu().numpy().view(np.uint64)]
        print(json.dumps(dict(what="frame %d (blurred over %d columns) at radius %d, %d sources" % (q, BLUR, RADIUS, len(src)), size="%dx%d" % (COLS, ROWS), channels=3,
                              reps=args.reps, launches=dict(deblur=rsdsfm.deblur_launches(ROWS, COLS, len(src)), renders=len(src) * rsdsfm.stabilize_window_launches(ROWS, COLS)),
                              deblur_frame_us=med(ts["b"]), deblur_frame_min_max_us=mm(ts["b"]), five_window_renders_us=med(ts["c"]), five_window_renders_min_max_us=mm(ts["c"]),
                              deblur_minus_renders_us=round(b - c, 1), per_neighbour_us=round((b - c) / (len(src) - 1), 1),
                              renders_spread_us=round(max(ts["c"]) - min(ts["c"]), 1), taus=taus, counts_unset_own_transferred=counts.cpu().numpy().tolist(),
                              mean_weight=round(float(wplane.float().mean().item()), 2))), flush=True)
        # (d) the clip at radius 2
        outs, omasks, ows = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], [u8() for _ in range(PAIRS)], [u8() for _ in range(PAIRS)]
        torch.cuda.synchronize()
        video = lambda: s.deblur_video_dev(p(d_frames[:PAIRS]), ROWS, COLS, 3, K, p(dms), p(Rs), p(Ts), r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p(outs), p(omasks),
                                           p(ows), radius=RADIUS)
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
                              us_per_output_frame=med(tv), min_max_us=mm(tv), counts_sum_unset_own_transferred=res["counts"].sum(axis=0).tolist(),
                              taus_of_frames_0_to_4=res["taus"][:5].tolist())), flush=True)


if __name__ == "__main__":
    main()
