"""Timing of the noise curve at 1280x720 BGR ("Noise curve"), one process, HIP events on the context's stream, medians of 20
repeated, warmed-up calls (tools/noise_time.py's protocol); the variants of a group alternate, so that all see the same machine:

  (a) rsdsfm_noise_curve_dev (one memset of 32 KB, the banded histogram launch, the nine-workgroup resolve launch) on the noisy frame, on a flat
      frame (every sample on one key: the contention path) and under an empty mask (no sample: the zeroing and the flush of the 32 KB alone),
      each beside rsdsfm_noise_level_dev on the same planes;
  (b) rsdsfm_denoise_accumulate_curve_dev beside rsdsfm_denoise_accumulate_auto_dev (one layer, first and last) and
      rsdsfm_denoise_spatial_curve_dev beside rsdsfm_denoise_spatial_auto_dev (search 2), on the same planes;
  (c) one rsdsfm_denoise_curve_frame_dev against rsdsfm_denoise_auto_frame_dev on the same five sources, without and with the top-up;
  (d) rsdsfm_denoise_curve_video_dev against rsdsfm_denoise_auto_video_dev per output frame, with the host arrays.

The expectation, stated before the run.  profiles/noise_time.txt has the noise level at 29.8 us on the noisy frame (histogram launch 21.2 us,
resolve 4.9 us), 22.8 us flat and 10.9 us under an empty mask.  The banded histogram does the same reads and the same twelve LDS atomics per
thread at most; what it adds is (1) zeroing and flushing 32 words per thread in place of 4: 64 KB of LDS traffic per workgroup, 512 cycles at
128 B per clock and CU, 14 workgroups per CU: about 3 us over the chip; (2) some sixty more VALU instructions per thread for the [1, 1, 1]
sums, well under 1 us; (3) an occupancy of four workgroups per CU (37 520 B of LDS) where the noise level's kernel is limited by nothing of
the kind; (4) more non-zero keys to flush with global atomics, a tile spanning one to three bands.  The resolve's nine workgroups run side by
side and the ninth reads eight times as much, 32 KB: no more than 1 us over the one-workgroup resolve.  So: the curve primitive within 10 us of
the noise level on the noisy and the flat frame, within 5 us under the empty mask.  The consumers form a 256-entry table per workgroup, some
hundred and fifty instructions per thread once, and read one LDS byte per pixel: within 3 us, or 3 %, of their auto twins.  The frame call
should differ from the auto frame call by the primitives' difference plus four accumulates' and the top-up's: within 25 us; the clip call per
frame likewise.  No time is gated.  Every line says what came out, and the last says whether the expectation held.  One JSON line per
measurement; the record is profiles/noise_curve_time.txt.

    python tools/noise_curve_time.py [--reps 20] [--clip-reps 3] [--warmup 3] > profiles/noise_curve_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

RADIUS = 2
NOISE = (2, 20)  # signal-dependent: the amplitude at byte 0 and at byte 255


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clip-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    import rsdsfm
    import rsdsfm_noise_curve as nc

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    frames, K = clip(rsdsfm, PAIRS + 1)
    rng = np.random.default_rng(5)
    amp = lambda f: NOISE[0] + ((NOISE[1] - NOISE[0]) * f.astype(np.int64) + 127) // 255
    frames = [np.clip(f.astype(np.int64) + rng.integers(-amp(f), amp(f) + 1), 0, 255).astype(np.uint8) for f in frames]  # sensor noise, per frame

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

    def warmed(calls, s):
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        return timed(calls, args.reps)

    med = lambda v: round(float(np.median(v)), 1)
    mm = lambda v: [round(min(v), 1), round(max(v), 1)]
    size = "%dx%d" % (COLS, ROWS)
    held = {}
    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        u8 = lambda: torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        p = lambda xs: [x.data_ptr() for x in xs]
        q = 2
        # (a) the primitive beside the noise level
        d_noisy, d_flat = up(frames[q]), up(np.full((ROWS, COLS, 3), 128, dtype=np.uint8))
        d_full, d_empty = up(np.ones((ROWS, COLS), dtype=np.uint8)), up(np.zeros((ROWS, COLS), dtype=np.uint8))
        d_hist, d_rec = torch.empty(1024, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int64, device=dev)
        d_hist8, d_curve = torch.empty(8192, dtype=torch.int32, device=dev), torch.empty(36, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        level = lambda img, mask: (lambda: s.noise_level_dev(img.data_ptr(), mask.data_ptr(), 3, ROWS, COLS, d_hist.data_ptr(), d_rec.data_ptr()))
        curve = lambda img, mask: (lambda: nc.noise_curve_dev(s, img.data_ptr(), mask.data_ptr(), 3, ROWS, COLS, d_hist8.data_ptr(), d_curve.data_ptr()))
        inputs = dict(noisy=(d_noisy, d_full), flat=(d_flat, d_full), empty=(d_noisy, d_empty))
        calls = {}
        for name, (img, mask) in inputs.items():
            calls["level " + name], calls["curve " + name] = level(img, mask), curve(img, mask)
        ts = warmed(calls, s)
        for name in inputs:
            calls["curve " + name]()
            s.synchronize()
            cv = d_curve.cpu().numpy().reshape(9, 4)
            a, b = ts["level " + name], ts["curve " + name]
            diff = round(float(np.median(b)) - float(np.median(a)), 1)
            held["primitive " + name] = diff <= (5.0 if name == "empty" else 10.0)
            print(json.dumps(dict(what="noise curve beside the noise level, %s" % name, size=size, channels=3, reps=args.reps, launches=nc.noise_curve_launches(),
                                  noise_level_us=med(a), noise_level_min_max_us=mm(a), noise_curve_us=med(b), noise_curve_min_max_us=mm(b), difference_us=diff,
                                  band_n=cv[:8, 0].tolist(), band_m=cv[:8, 1].tolist(), all_n_m=cv[8, :2].tolist())), flush=True)
        # (b) the consumers beside their auto twins, on the noisy frame's curve and record
        curve(d_noisy, d_full)()
        level(d_noisy, d_full)()
        d_layer, d_cnt = up(frames[q + 1]), torch.zeros(3, dtype=torch.int64, device=dev)
        d_lmask = up(np.ones((ROWS, COLS), dtype=np.uint8))  # the layer's mask is a plane of its own: the call refuses the reference's
        o_img, o_mask, o_w, o_sup = torch.empty_like(d_noisy), u8(), u8(), u8()
        torch.cuda.synchronize()
        acc = (d_noisy.data_ptr(), d_full.data_ptr(), d_layer.data_ptr(), d_lmask.data_ptr(), 3, ROWS, COLS, None, True, True)
        outs = dict(d_image_out=o_img.data_ptr(), d_mask_out=o_mask.data_ptr(), d_weight=o_w.data_ptr(), d_counts3=d_cnt.data_ptr())
        top = (d_noisy.data_ptr(), d_full.data_ptr(), None, 3, ROWS, COLS)
        calls = {"accumulate auto": lambda: s.denoise_accumulate_auto_dev(*acc, d_rec.data_ptr(), **outs),
                 "accumulate curve": lambda: nc.denoise_accumulate_curve_dev(s, *acc, d_curve.data_ptr(), **outs),
                 "top-up auto": lambda: s.denoise_spatial_auto_dev(*top, d_rec.data_ptr(), o_img.data_ptr(), o_sup.data_ptr(), d_cnt.data_ptr()),
                 "top-up curve": lambda: nc.denoise_spatial_curve_dev(s, *top, d_curve.data_ptr(), o_img.data_ptr(), o_sup.data_ptr(), d_cnt.data_ptr())}
        ts = warmed(calls, s)
        for kind in ("accumulate", "top-up"):
            a, b = ts[kind + " auto"], ts[kind + " curve"]
            diff = float(np.median(b)) - float(np.median(a))
            held["consumer " + kind] = diff <= max(3.0, 0.03 * float(np.median(a)))
            print(json.dumps(dict(what="%s with the curve beside its auto twin" % kind, size=size, channels=3, reps=args.reps, auto_us=med(a), auto_min_max_us=mm(a), curve_us=med(b),
                                  curve_min_max_us=mm(b), difference_us=round(diff, 1))), flush=True)
        # the clip, solved once
        d_frames = [up(f) for f in frames]
        mk = lambda shape, dt: [torch.empty(shape, dtype=dt, device=dev) for _ in range(PAIRS)]
        dms, flows, Rs, Ts = mk(ROWS * COLS, torch.float64), mk((ROWS, COLS, 2), torch.float64), mk(ROWS * 9, torch.float64), mk(ROWS * 3, torch.float64)
        stabs, smasks = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], mk((ROWS, COLS), torch.uint8)
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        r = s.stabilize_video_dev(p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks), trials=50, tol=0.05)
        s.synchronize()
        _, _, M0, m0, _, _ = rsdsfm.retime_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], float(q), nsources=PAIRS)
        nb, _, Mn, mn = rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"][:PAIRS], q, RADIUS)
        src = [q] + [int(n) for n in nb]
        M, m = np.concatenate([M0, Mn]), np.concatenate([m0, mn])
        pick = lambda xs: [xs[n].data_ptr() for n in src]
        out, t_mask, t_w, sup = torch.empty_like(d_frames[0]), u8(), u8(), u8()
        counts6 = torch.zeros(6, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        # (c) the frame calls
        fargs = (pick(d_frames), 3, pick(dms), pick(Rs), pick(Ts), K, ROWS, COLS, M, m, out.data_ptr(), t_mask.data_ptr(), t_w.data_ptr())
        calls = dict(auto=lambda: s.denoise_auto_frame_dev(*fargs, None, counts6.data_ptr(), d_rec.data_ptr()),
                     curve=lambda: nc.denoise_curve_frame_dev(s, *fargs, None, counts6.data_ptr(), d_curve.data_ptr()),
                     auto_both=lambda: s.denoise_auto_frame_dev(*fargs, sup.data_ptr(), counts6.data_ptr(), d_rec.data_ptr(), spatial=True),
                     curve_both=lambda: nc.denoise_curve_frame_dev(s, *fargs, sup.data_ptr(), counts6.data_ptr(), d_curve.data_ptr(), spatial=True))
        tf = warmed(calls, s)
        calls["curve"]()
        s.synchronize()
        cv = d_curve.cpu().numpy().reshape(9, 4)
        lut = nc.noise_curve_strengths(cv.view(np.uint64))
        d1 = float(np.median(tf["curve"])) - float(np.median(tf["auto"]))
        d2 = float(np.median(tf["curve_both"])) - float(np.median(tf["auto_both"]))
        held["frame"], held["frame with top-up"] = d1 <= 25.0, d2 <= 25.0
        print(json.dumps(dict(what="frame %d at radius %d, %d sources" % (q, RADIUS, len(src)), size=size, channels=3, reps=args.reps,
                              launches=dict(auto=rsdsfm.denoise_auto_frame_launches(ROWS, COLS, len(src)), curve=nc.denoise_curve_frame_launches(ROWS, COLS, len(src)),
                                            curve_both=nc.denoise_curve_frame_launches(ROWS, COLS, len(src), True)),
                              denoise_auto_frame_us=med(tf["auto"]), denoise_auto_frame_min_max_us=mm(tf["auto"]), denoise_curve_frame_us=med(tf["curve"]),
                              denoise_curve_frame_min_max_us=mm(tf["curve"]), difference_us=round(d1, 1), denoise_auto_frame_with_top_up_us=med(tf["auto_both"]),
                              denoise_curve_frame_with_top_up_us=med(tf["curve_both"]), difference_with_top_up_us=round(d2, 1), band_m=cv[:8, 1].tolist(), all_m=int(cv[8, 1]),
                              strength_min_max=[int(lut.min()), int(lut.max())])), flush=True)
        # (d) the clip calls per output frame
        outs_, omasks, ows = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], [u8() for _ in range(PAIRS)], [u8() for _ in range(PAIRS)]
        torch.cuda.synchronize()
        clip_args = (p(d_frames[:PAIRS]), ROWS, COLS, 3, K, p(dms), p(Rs), p(Ts), r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p(outs_), p(omasks), p(ows))
        videos = dict(auto=lambda: s.denoise_auto_video_dev(*clip_args, radius=RADIUS), curve=lambda: nc.denoise_curve_video_dev(s, *clip_args, radius=RADIUS))
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
        d3 = float(np.median(tv["curve"])) - float(np.median(tv["auto"]))
        held["clip per frame"] = d3 <= 25.0
        print(json.dumps(dict(what="clip at radius %d" % RADIUS, size=size, pairs=PAIRS, output_frames=PAIRS, reps=args.clip_reps,
                              denoise_auto_video_us_per_frame=med(tv["auto"]), denoise_auto_video_min_max_us=mm(tv["auto"]), denoise_curve_video_us_per_frame=med(tv["curve"]),
                              denoise_curve_video_min_max_us=mm(tv["curve"]), difference_us_per_frame=round(d3, 1),
                              noise_m_per_frame=res["curve"]["curves"][:, 8, 1].tolist(), band_0_and_7_m_per_frame=res["curve"]["curves"][:, [0, 7], 1].tolist())), flush=True)
        print(json.dumps(dict(what="expectation: the primitive within 10 us of the noise level (5 us under an empty mask), the consumers within 3 us or 3 % of their auto twins, "
                                   "the frame and clip calls within 25 us of the auto calls", held=held, all_held=all(held.values()))), flush=True)


if __name__ == "__main__":
    main()
