"""Timing of the sharpness transfer per scanline band at 1280x720 BGR ("Sharpness per scanline band"), one process, HIP events
on the context's stream, medians over repeated, warmed-up calls (tools/erase_time.py's protocol); the variants of a group alternate, so that all
see the same machine.  band_rows = 48: 15 bands.

  (a) rsdsfm_deblur_band_sharpness_dev beside rsdsfm_deblur_sharpness_dev on the same reference (its lower half box-blurred over 5 columns) and
      layer (90 % of the layer set);
  (b) rsdsfm_deblur_band_accumulate_dev as a mid, a first and a last launch (the last with the weight plane and the counters) with every band's tau
      16, and as a mid launch with every band's tau 0 (it returns behind the records), beside rsdsfm_deblur_accumulate_dev in the same places on the
      same planes with tau 16 and tau 0;
  (c) one rsdsfm_deblur_frame_dev at radius 2 (frame 2 of tools/deblur_time.py's solved clip, that frame's lower half box-blurred, five sources,
      on the smoothed path) with and without band_rows;
  (d) rsdsfm_deblur_video_dev at radius 2 on the 16-pair clip with and without band_rows, per output frame, with the counts and the taus.
The expectation from the code, to confirm or refute: the same bytes and launches as the unbanded calls and two more 64-bit divisions per workgroup,
so times inside the unbanded calls' spread.  No time is gated.  One JSON line per measurement; the record is profiles/deblur_bands_time.txt.

    python tools/deblur_bands_time.py [--reps 20] [--clip-reps 5] [--warmup 3] > profiles/deblur_bands_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deblur_time import BLUR, BLURRED, RADIUS, box_blur  # noqa: E402
from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

BAND_ROWS = 48
NB = -(-ROWS // BAND_ROWS)


def half_blur(frame):
    """the frame with its lower half box-blurred over BLUR columns"""
    out = frame.copy()
    out[ROWS // 2:] = box_blur(frame, BLUR)[ROWS // 2:]
    return out


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
    frames = [half_blur(f) if j == BLURRED else f for j, f in enumerate(frames)]  # the blur before the noise
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
            print(json.dumps(dict(what=name, size="%dx%d" % (COLS, ROWS), channels=3, band_rows=BAND_ROWS, reps=len(v), launches=launches, us=med(v), min_max_us=mm(v))),
                  flush=True)

    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        u8 = lambda: torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        # (a) the band sharpness launch beside the sharpness launch
        sharp_frame = frames[0]
        ref = half_blur(sharp_frame)
        mask_set = np.ones((ROWS, COLS), dtype=np.uint8)
        mask_set[:, :COLS // 10] = 0  # a band along one edge, as a moved camera leaves it
        d_ref, d_full, d_set = up(ref), up(np.ones((ROWS, COLS), dtype=np.uint8)), up(mask_set)
        d_near = up(np.clip(sharp_frame.astype(np.int64) + rng.integers(-5, 6, size=ref.shape), 0, 255).astype(np.uint8))
        d_cells = torch.zeros((ROWS, COLS, 4), dtype=torch.int16, device=dev)
        d_rec, d_T, d_TB = torch.zeros(8, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros((NB, 4), dtype=torch.int64, device=dev)
        up64 = lambda words: torch.from_numpy(np.array(words, dtype=np.uint64).view(np.int64)).to(dev)
        d_T16, d_T0 = up64([5000, 1000, 2000, 0]), up64([5000, 1000, 1000, 0])  # tau = 16 and tau = 0
        d_B16, d_B0 = up64([[5000, 1000, 2000, 0]] * NB), up64([[5000, 1000, 1000, 0]] * NB)
        out, mask, wplane = torch.empty_like(d_ref), u8(), u8()
        counts = torch.zeros(3, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        planes = (d_ref.data_ptr(), d_full.data_ptr(), d_near.data_ptr(), d_set.data_ptr(), 3, ROWS, COLS)
        s.seam_overlap_sums_dev(*planes, d_rec.data_ptr())
        calls = {"band sharpness, 90 % set": lambda: s.deblur_band_sharpness_dev(*planes, BAND_ROWS, d_TB.data_ptr(), d_rec.data_ptr()),
                 "sharpness, 90 % set": lambda: s.deblur_sharpness_dev(*planes, d_T.data_ptr(), d_rec.data_ptr())}
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        report(timed(calls, args.reps))
        T, TB = d_T.cpu().numpy().view(np.uint64), d_TB.cpu().numpy().view(np.uint64)
        print(json.dumps(dict(what="the records of (a)", pairs_AR_AL=T[:3].tolist(), tau=rsdsfm.deblur_tau(T), band_taus=rsdsfm.deblur_band_taus(TB).tolist(),
                              bands_sum_to_the_record=bool((TB.sum(axis=0) == T).all()))), flush=True)

        # (b) the band accumulate beside the accumulate
        extra = lambda extras: dict(d_image_out=out.data_ptr(), d_mask_out=mask.data_ptr(), d_weight=wplane.data_ptr() if extras else None,
                                    d_counts3=counts.data_ptr() if extras else None)

        def banded(first, last, extras, d_sharp):
            return lambda: s.deblur_band_accumulate_dev(*planes, BAND_ROWS, d_cells.data_ptr(), first, last, d_sharp.data_ptr(), d_rec.data_ptr(), **extra(extras))

        def plain(first, last, extras, d_sharp):
            return lambda: s.deblur_accumulate_dev(*planes, d_cells.data_ptr(), first, last, d_sharp.data_ptr(), d_rec.data_ptr(), **extra(extras))

        # a mid launch adds to the cells every time it runs: a first launch (untimed) sets them again in front of every repetition
        first = plain(True, False, False, d_T16)
        calls = {"band accumulate: first, taus 16": banded(True, False, False, d_B16), "accumulate: first, tau 16": first,
                 "band accumulate: mid, taus 16": banded(False, False, False, d_B16), "accumulate: mid, tau 16": plain(False, False, False, d_T16),
                 "band accumulate: mid, taus 0 (returns behind the records)": banded(False, False, False, d_B0),
                 "accumulate: mid, tau 0 (returns behind the record)": plain(False, False, False, d_T0),
                 "band accumulate: last, taus 16, weight plane and counters": banded(False, True, True, d_B16),
                 "accumulate: last, tau 16, weight plane and counters": plain(False, True, True, d_T16)}
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
        # (c) the half-blurred frame at radius 2, with and without bands
        q = BLURRED
        _, _, M0, m0, _, _ = rsdsfm.retime_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], float(q), nsources=PAIRS)
        nb, _, Mn, mn = rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"][:PAIRS], q, RADIUS)
        src = [q] + [int(n) for n in nb]
        M, m = np.concatenate([M0, Mn]), np.concatenate([m0, mn])
        pick = lambda xs: [xs[n].data_ptr() for n in src]
        d_records = torch.zeros((len(src) - 1, NB, 4), dtype=torch.int64, device=dev)

        def frame(band_rows):
            return lambda: s.deblur_frame_dev(pick(d_frames), 3, pick(dms), pick(Rs), pick(Ts), K, ROWS, COLS, M, m, out.data_ptr(), mask.data_ptr(), wplane.data_ptr(),
                                              counts.data_ptr(), d_records.data_ptr(), band_rows=band_rows)

        calls = {"frame %d (lower half blurred) at radius %d, %d sources, band_rows %d" % (q, RADIUS, len(src), BAND_ROWS): frame(BAND_ROWS),
                 "frame %d (lower half blurred) at radius %d, %d sources, no bands" % (q, RADIUS, len(src)): frame(None)}
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        report(timed(calls, args.reps), launches=rsdsfm.deblur_launches(ROWS, COLS, len(src)))
        frame(None)()
        s.synchronize()
        plain_taus = [rsdsfm.deblur_tau(T) for T in d_records.cpu().numpy().view(np.uint64).reshape(-1, 4)[:len(src) - 1]]
        plain_counts = counts.cpu().numpy().tolist()
        frame(BAND_ROWS)()
        s.synchronize()
        print(json.dumps(dict(what="the taus of (c)", taus=plain_taus, counts_unset_own_transferred=plain_counts,
                              band_taus=[rsdsfm.deblur_band_taus(T).tolist() for T in d_records.cpu().numpy().view(np.uint64)],
                              banded_counts_unset_own_transferred=counts.cpu().numpy().tolist())), flush=True)
        # (d) the clip at radius 2, with and without bands
        outs, omasks, ows = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], [u8() for _ in range(PAIRS)], [u8() for _ in range(PAIRS)]
        torch.cuda.synchronize()

        def video(band_rows):
            return lambda: s.deblur_video_dev(p(d_frames[:PAIRS]), ROWS, COLS, 3, K, p(dms), p(Rs), p(Ts), r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], p(outs), p(omasks),
                                              p(ows), radius=RADIUS, band_rows=band_rows)

        calls = {"clip at radius %d, band_rows %d" % (RADIUS, BAND_ROWS): video(BAND_ROWS), "clip at radius %d, no bands" % RADIUS: video(None)}
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        tv, res = {k_: [] for k_ in calls}, {}
        for _ in range(args.clip_reps):
            for name, fn in calls.items():
                e0, e1 = event_pair()
                e0.record(stream)
                res[name] = fn()
                e1.record(stream)
                e1.synchronize()
                tv[name].append(e0.elapsed_time(e1) * 1e3 / PAIRS)
        for name, v in tv.items():
            print(json.dumps(dict(what=name, size="%dx%d" % (COLS, ROWS), pairs=PAIRS, output_frames=PAIRS, reps=args.clip_reps, us_per_output_frame=med(v), min_max_us=mm(v),
                                  counts_sum_unset_own_transferred=res[name]["counts"].sum(axis=0).tolist(), taus_of_frame_2=res[name]["taus"][BLURRED].tolist())), flush=True)


if __name__ == "__main__":
    main()
