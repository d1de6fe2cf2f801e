"""Timing of the colour-consistent plate at 1280x720 BGR ("Colour-consistent plate"), one process, HIP events on the context's
stream, medians over repeated, warmed-up calls (tools/plate_time.py's protocol and inputs): rsdsfm_plate_medoid_dev and rsdsfm_plate_median_dev at
3, 5 and 15 sources (2, 4 and 14 layers, each 90 - 97.5 % set and within +-5 of the reference), with the votes, the flag plane and the counters and
without any of them.  All twelve variants alternate inside every repetition, so that all see the same machine: the median's time in the same
run is the yardstick, no time is gated.  The bytes are the same for both estimators -- at N sources N (3 + 1) B read and 3 + 1 (+ 1 + 1) B written
per pixel --; what differs is the selection: N (N - 1) v_sad_u8 per pixel against the median's sorting network.  Every line says what came out.
One JSON line per measurement; the record is profiles/plate_medoid_time.txt.

    python tools/plate_medoid_time.py [--reps 30] [--warmup 3] > profiles/plate_medoid_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import COLS, ROWS, clip  # noqa: E402  (the stabiliser's frame and sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    frames, _ = clip(rsdsfm, 2)
    rng = np.random.default_rng(5)
    ref = np.clip(frames[0].astype(np.int64) + rng.integers(-6, 7, size=frames[0].shape), 0, 255).astype(np.uint8)  # sensor noise

    med = lambda v: round(float(np.median(v)), 1)
    mm = lambda v: [round(min(v), 1), round(max(v), 1)]
    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        u8 = lambda: torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
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
        outs = {e: (torch.empty_like(d_ref), u8(), u8(), u8(), torch.zeros(4, dtype=torch.int64, device=dev)) for e in ("medoid", "median")}
        torch.cuda.synchronize()
        ptr = lambda xs: [x.data_ptr() for x in xs]

        def call(estimator, L, extras):
            fn = s.plate_medoid_dev if estimator == "medoid" else s.plate_median_dev
            out, mask, votes, moving, counts = outs[estimator]
            li, lm = ptr(d_layers[:L]), ptr(d_masks[:L])
            return lambda: fn(d_ref.data_ptr(), d_full.data_ptr(), li, lm, 3, ROWS, COLS, out.data_ptr(), mask.data_ptr(), votes.data_ptr() if extras else None,
                              moving.data_ptr() if extras else None, counts.data_ptr() if extras else None, d_recs.data_ptr())

        calls = {(e, nsrc, extras): call(e, nsrc - 1, extras) for nsrc in (3, 5, 15) for extras in (True, False) for e in ("medoid", "median")}
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        ts = {k: [] for k in calls}
        for _ in range(args.reps):
            for key, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ts[key].append(e0.elapsed_time(e1) * 1e3)
        for nsrc in (3, 5, 15):
            for extras in (True, False):
                a, b = ts[("medoid", nsrc, extras)], ts[("median", nsrc, extras)]
                calls[("medoid", nsrc, extras)]()
                calls[("median", nsrc, extras)]()
                s.synchronize()
                differ = int((outs["medoid"][0] != outs["median"][0]).any(dim=-1).sum().item())
                print(json.dumps(dict(what="%d sources, %s" % (nsrc, "votes, flag plane and counters" if extras else "plate and mask only"), size="%dx%d" % (COLS, ROWS),
                                      channels=3, reps=args.reps, launches=1, medoid_us=med(a), medoid_min_max_us=mm(a), median_us=med(b), median_min_max_us=mm(b),
                                      medoid_over_median=round(float(np.median(a)) / float(np.median(b)), 2), pairs_per_pixel=nsrc * (nsrc - 1) // 2,
                                      bytes_per_pixel="%d read + %d written" % (4 * nsrc, 6 if extras else 4), pixels_where_the_plates_differ=differ,
                                      medoid_counts_unset_static_moving_undecided=outs["medoid"][4].cpu().numpy().tolist() if extras else None)), flush=True)


if __name__ == "__main__":
    main()
