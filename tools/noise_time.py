"""Timing of the noise level at 1280x720 BGR ("Noise level"), one process, HIP events on the context's stream, medians of 20
repeated, warmed-up calls (tools/denoise_time.py's protocol); the variants of a group alternate, so that all see the same machine:

  (a) rsdsfm_noise_level_dev (one memset, the histogram launch, the resolve launch) on the noisy frame, on a flat frame (every sample in bin 0:
      the contention path) and under an empty mask (no image byte is read, no sample); the same call on a 2 x 2 frame -- the memset, a
      one-workgroup histogram launch and the resolve, i.e. everything but the histogram's work: the floor, and the nearest the public surface
      comes to the resolve launch alone --; and beside them rsdsfm_seam_overlap_sums_dev on the same frame, the existing launch that reads two
      images and adds a record with atomics: the yardstick;
  (b) one rsdsfm_denoise_auto_frame_dev against rsdsfm_denoise_frame_dev on the same five sources, and with the top-up against
      rsdsfm_denoise_spatial_frame_dev;
  (c) rsdsfm_denoise_auto_video_dev against rsdsfm_denoise_video_dev per output frame, with the host arrays (one copy and one wait at the end).

The expectation, stated before the run.  Bytes: the histogram launch reads 3 + 1 B per pixel, 3.7 MB at this size, one or two microseconds of
HBM time; it is not bound by memory.  Per thread some 600 VALU instructions (18 clipped-byte tests, 54 byte extractions, the pairwise combine of
twelve bins): 3 600 waves on 1 024 SIMDs at 4 cycles per wave-instruction and 2.4 GHz give about 3.5 us.  The unknown is the LDS-atomic rate,
which this project has never measured: 3 072 atomics per workgroup on the noisy frame, spread over some tens of bins; 256 per workgroup, all on
one address, on the flat frame (after the combine in registers).  If an LDS atomic wave-instruction costs of the order of 64 cycles whatever its
addresses, twelve per wave are 768 cycles per wave, 1.1 us over the chip: the whole call should then lie within 10 us of its floor on the
noisy frame, the flat frame should cost no more than the noisy one, and the empty mask should sit at the floor.  The frame and clip calls
should differ from the existing ones by about one primitive call.  No time is gated.  Every line says what came out, and the last says whether
the expectation held.  One JSON line per measurement; the record is profiles/noise_time.txt.

    python tools/noise_time.py [--reps 20] [--clip-reps 3] [--warmup 3] > profiles/noise_time.txt

The public call enqueues the memset and both launches, so events around it cannot tell the histogram launch from the resolve launch.  A kernel
trace can: rocprofv3 --kernel-trace --stats -- python tools/noise_time.py --primitive-only noisy (or flat, or empty) runs the one call
warmup + reps times and the trace's statistics give each kernel's own mean (the record has them below the tool's lines).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

RADIUS = 2
NOISE = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clip-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--primitive-only", choices=["noisy", "flat", "empty"], default=None,
                    help="only rsdsfm_noise_level_dev on that input, nothing printed: for a kernel trace (rocprofv3 --kernel-trace --stats), which gives the two launches apart")
    args = ap.parse_args()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    frames, K = clip(rsdsfm, PAIRS + 1)
    rng = np.random.default_rng(5)
    frames = [np.clip(f.astype(np.int64) + rng.integers(-NOISE, NOISE + 1, size=f.shape), 0, 255).astype(np.uint8) for f in frames]  # sensor noise, per frame

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
        q = 2
        # (a) the primitive alone
        d_noisy, d_flat = up(frames[q]), up(np.full((ROWS, COLS, 3), 128, dtype=np.uint8))
        d_full, d_empty = up(np.ones((ROWS, COLS), dtype=np.uint8)), up(np.zeros((ROWS, COLS), dtype=np.uint8))
        d_tiny, d_tiny_mask = up(np.full((2, 2, 3), 128, dtype=np.uint8)), up(np.ones((2, 2), dtype=np.uint8))
        d_other, d_source = up(frames[q + 1]), up(np.ones((ROWS, COLS), dtype=np.uint8))
        d_hist, d_rec, d_sums = torch.empty(1024, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int64, device=dev), torch.empty(8, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        level = lambda img, mask, rows=ROWS, cols=COLS: (lambda: s.noise_level_dev(img.data_ptr(), mask.data_ptr(), 3, rows, cols, d_hist.data_ptr(), d_rec.data_ptr()))
        if args.primitive_only:
            fn = dict(noisy=level(d_noisy, d_full), flat=level(d_flat, d_full), empty=level(d_noisy, d_empty))[args.primitive_only]
            for _ in range(args.warmup + args.reps):
                fn()
            s.synchronize()
            return
        calls = {"noise level, the noisy frame": level(d_noisy, d_full), "noise level, a flat frame (one bin)": level(d_flat, d_full),
                 "noise level, an empty mask": level(d_noisy, d_empty), "noise level, a 2 x 2 frame (the floor)": level(d_tiny, d_tiny_mask, 2, 2),
                 "seam overlap sums (the yardstick)": lambda: s.seam_overlap_sums_dev(d_noisy.data_ptr(), d_source.data_ptr(), d_other.data_ptr(), d_full.data_ptr(), 3, ROWS,
                                                                                     COLS, d_sums.data_ptr())}
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        ts = timed(calls, args.reps)
        for name, fn in calls.items():
            rec = None
            if name.startswith("noise"):
                fn()
                s.synchronize()
                rec = d_rec.cpu().numpy().tolist()
            print(json.dumps(dict(what=name, size=size if "2 x 2" not in name else "2x2", channels=3, reps=args.reps, launches=rsdsfm.noise_level_launches() if rec else 1,
                                  us=med(ts[name]), min_max_us=mm(ts[name]), record_n_m_sigma_q8=rec[:3] if rec else None)), flush=True)
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
        counts3, counts6 = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(6, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        # (b) the frame calls
        fargs = (pick(d_frames), 3, pick(dms), pick(Rs), pick(Ts), K, ROWS, COLS, M, m, out.data_ptr(), t_mask.data_ptr(), t_w.data_ptr())
        calls = dict(temporal=lambda: s.denoise_frame_dev(*fargs, counts3.data_ptr()),
                     auto=lambda: s.denoise_auto_frame_dev(*fargs, None, counts6.data_ptr(), d_rec.data_ptr()),
                     both=lambda: s.denoise_spatial_frame_dev(*fargs, sup.data_ptr(), counts6.data_ptr()),
                     auto_both=lambda: s.denoise_auto_frame_dev(*fargs, sup.data_ptr(), counts6.data_ptr(), d_rec.data_ptr(), spatial=True))
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        tf = timed(calls, args.reps)
        calls["auto"]()
        s.synchronize()
        rec = d_rec.cpu().numpy().tolist()
        print(json.dumps(dict(what="frame %d at radius %d, %d sources" % (q, RADIUS, len(src)), size=size, channels=3, reps=args.reps,
                              launches=dict(temporal=rsdsfm.denoise_launches(ROWS, COLS, len(src)), auto=rsdsfm.denoise_auto_frame_launches(ROWS, COLS, len(src)),
                                            both=rsdsfm.denoise_spatial_frame_launches(ROWS, COLS, len(src)), auto_both=rsdsfm.denoise_auto_frame_launches(ROWS, COLS, len(src), True)),
                              denoise_frame_us=med(tf["temporal"]), denoise_frame_min_max_us=mm(tf["temporal"]), denoise_auto_frame_us=med(tf["auto"]),
                              denoise_auto_frame_min_max_us=mm(tf["auto"]), difference_us=round(float(np.median(tf["auto"])) - float(np.median(tf["temporal"])), 1),
                              denoise_spatial_frame_us=med(tf["both"]), denoise_auto_frame_with_top_up_us=med(tf["auto_both"]),
                              difference_with_top_up_us=round(float(np.median(tf["auto_both"])) - float(np.median(tf["both"])), 1), record_n_m_sigma_q8=rec[:3],
                              strength=rsdsfm.noise_strength(rec[0], rec[1]))), flush=True)
        # (c) the clip calls per output frame
        outs, omasks, ows = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], [u8() for _ in range(PAIRS)], [u8() for _ in range(PAIRS)]
        torch.cuda.synchronize()
        clip_args = (p(d_frames[:PAIRS]), ROWS, COLS, 3, K, p(dms), p(Rs), p(Ts), r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p(outs), p(omasks), p(ows))
        videos = dict(temporal=lambda: s.denoise_video_dev(*clip_args, radius=RADIUS), auto=lambda: s.denoise_auto_video_dev(*clip_args, radius=RADIUS))
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
                              denoise_video_us_per_frame=med(tv["temporal"]), denoise_video_min_max_us=mm(tv["temporal"]), denoise_auto_video_us_per_frame=med(tv["auto"]),
                              denoise_auto_video_min_max_us=mm(tv["auto"]), noise_m_per_frame=res["auto"]["noise"][:, 1].tolist())), flush=True)
        # the expectation against what came out
        g = {k_: float(np.median(v)) for k_, v in ts.items()}
        floor = g["noise level, a 2 x 2 frame (the floor)"]
        noisy, flat, empty = g["noise level, the noisy frame"], g["noise level, a flat frame (one bin)"], g["noise level, an empty mask"]
        print(json.dumps(dict(what="expectation", floor_us=round(floor, 1), histogram_work_us=dict(noisy=round(noisy - floor, 1), flat=round(flat - floor, 1), empty=round(empty - floor, 1)),
                              noisy_within_10_us_of_the_floor=noisy - floor <= 10.0, flat_no_more_than_noisy=flat <= noisy, empty_at_the_floor=empty - floor <= 3.0,
                              yardstick_us=round(g["seam overlap sums (the yardstick)"], 1))), flush=True)


if __name__ == "__main__":
    main()
