"""Timing of the trajectory calls at 1280x720 ("Trajectory"), one process, HIP events on the context's stream, medians over
repeated, warmed-up calls, the variants of one comparison alternating:

  (1) rsdsfm_link_pairs_dev: the 15 links of 16 pairs in one call, with 11-bit digits (six radix passes) and with 8-bit digits (eight), against
      the HBM floor of the bytes they move (link_kernels.hip: 40 B per pixel and link for the ratio pass, 8 B for each radix pass and for the
      agree pass, at the 8.0 TB/s peak).  The call ends with its one copy and wait, so its time includes them.  The maps are synthetic (a
      smooth scene, 60 % of the pixels with a depth, as a solve with outliers leaves them); both widths must return the same records;
  (2) rsdsfm_clip_points_dev over 16 pairs, in place, against its floor (12 B read + 12 B written per pixel);
  (3) rsdsfm_solve_video_dev and rsdsfm_solve_video_linked_dev over 16 pairs at B = 8, per pair, with the spread of each one's repetitions.
One JSON line per measurement; the record is profiles/link_time.txt.

    python tools/link_time.py [--reps 20] [--clip-reps 5] [--warmup 2] > profiles/link_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS, PAIRS, BATCH = 720, 1280, 16, 8
HBM_PEAK = 8.0e12  # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clip-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    npix = ROWS * COLS
    K = (0.75 * COLS, 0.75 * COLS, 0.5 * COLS, 0.5 * ROWS)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(ROWS, COLS, K, v, w, k, 0.8, _model_only=True)
    sc = 5.0 / np.abs(f0).max()
    v, w = v * sc, w * sc

    def once(s, fn, wait):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        if wait:
            s.synchronize()  # (solve_video_dev returns with its lanes still running)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternating(s, fns, reps, wait=False):
        """ms of every fn, repetition by repetition in turn; per fn (median, min, max)"""
        for _ in range(args.warmup):
            for fn in fns:
                fn()
                s.synchronize()
        ts = [[] for _ in fns]
        for _ in range(reps):
            for fn, acc in zip(fns, ts):
                acc.append(once(s, fn, wait))
        return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]

    with torch.cuda.device(dev), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        # (1) the links alone
        r = np.random.default_rng(1)
        field = torch.from_numpy(np.ascontiguousarray(f0 * sc)).to(dev)
        Z = rsdsfm.synth.scene_depth(ROWS, COLS)
        maps = []
        for q in range(PAIRS):
            z = Z * (1.0 + 0.1 * q) * np.exp(r.normal(0.0, 0.02, (ROWS, COLS)))
            z[r.uniform(size=(ROWS, COLS)) < 0.4] = 0.0
            maps.append(torch.from_numpy(np.ascontiguousarray(z.T)).to(dev))
        torch.cuda.synchronize()
        fp, mp = [field.data_ptr()] * PAIRS, [m.data_ptr() for m in maps]
        vs, ws, ks = [v / np.linalg.norm(v)] * PAIRS, [w] * PAIRS, [0.0] * PAIRS
        res = {}
        link = lambda bits: (lambda: res.__setitem__(bits, s.link_pairs_dev(fp, mp, vs, ws, ks, ROWS, COLS, K, 0.8, radix_bits=bits)))
        t11, t8 = alternating(s, [link(11), link(8)], args.reps)
        for bits, t in ((11, t11), (8, t8)):
            passes = -(-64 // bits)
            bytes_px = 40 + 8 * passes + 8
            floor_us = bytes_px * npix * (PAIRS - 1) / HBM_PEAK * 1e6
            print(json.dumps(dict(what="links", size="%dx%d" % (COLS, ROWS), links=PAIRS - 1, radix_bits=bits, passes=passes, launches=2 + 2 * passes,
                                  us=round(t[0] * 1e3, 1), min_max_us=[round(t[1] * 1e3, 1), round(t[2] * 1e3, 1)], us_per_link=round(t[0] * 1e3 / (PAIRS - 1), 1),
                                  bytes_per_pixel_and_link=bytes_px, hbm_floor_us=round(floor_us, 1), over_floor=round(t[0] * 1e3 / floor_us, 2),
                                  mean_correspondences=int(np.mean([x["n"] for x in res[bits]])), same_records=res[8] == res[11])), flush=True)
        # (2) the clip's points
        pts = [torch.randn((ROWS, COLS, 3), dtype=torch.float32, device=dev) for _ in range(PAIRS)]
        pp = [p.data_ptr() for p in pts]
        ch = rsdsfm.chain_clip(res[11], vs, ws, 0.8)
        torch.cuda.synchronize()
        t = alternating(s, [lambda: s.clip_points_dev(pp, pp, ROWS, COLS, ch["scales"], ch["A"], ch["c"])], args.reps)[0]
        floor_us = 24 * npix * PAIRS / HBM_PEAK * 1e6
        print(json.dumps(dict(what="clip points", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, us=round(t[0] * 1e3, 1), min_max_us=[round(t[1] * 1e3, 1), round(t[2] * 1e3, 1)],
                              bytes_per_pixel_and_pair=24, hbm_floor_us=round(floor_us, 1), over_floor=round(t[0] * 1e3 / floor_us, 2))), flush=True)
        del pts, maps
        # (3) the clip
        frames, _, _ = rsdsfm.synth.render_sequence(PAIRS + 1, ROWS, COLS, K, v, w, k, 0.8, seed=1)
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        dms = [torch.empty(npix, dtype=torch.float64, device=dev) for _ in range(PAIRS)]
        fields = [torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev) for _ in range(PAIRS)]
        fr, mp, fl = [x.data_ptr() for x in d_frames], [x.data_ptr() for x in dms], [x.data_ptr() for x in fields]
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        solve = lambda: res.__setitem__("plain", s.solve_video_dev(fr, ROWS, COLS, 3, K, 0.8, mp, d_flows=fl, trials=50, tol=0.05))
        linked = lambda: res.__setitem__("linked", s.solve_video_linked_dev(fr, ROWS, COLS, 3, K, 0.8, mp, fl, trials=50, tol=0.05))
        c, d = alternating(s, [solve, linked], args.clip_reps, wait=True)
        lk = res["linked"]
        print(json.dumps(dict(what="clip", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, batch=BATCH, solve_video_ms_per_pair=round(c[0] / PAIRS, 3),
                              solve_video_min_max_ms=[round(c[1] / PAIRS, 3), round(c[2] / PAIRS, 3)], solve_video_spread_percent=round(100.0 * (c[2] - c[1]) / c[0], 2),
                              linked_ms_per_pair=round(d[0] / PAIRS, 3), linked_min_max_ms=[round(d[1] / PAIRS, 3), round(d[2] / PAIRS, 3)],
                              linked_spread_percent=round(100.0 * (d[2] - d[1]) / d[0], 2), linked_over_plain=round(d[0] / c[0], 4),
                              linked_minus_plain_us_per_pair=round((d[0] - c[0]) / PAIRS * 1e3, 1),
                              added_cost_inside_plain_spread=bool(d[0] - c[0] <= c[2] - c[1]),
                              mean_correspondences=int(np.mean([x["n"] for x in lk["links"]])), broken=int(lk["broken"].sum()),
                              scales_min_max=[round(float(lk["scales"].min()), 4), round(float(lk["scales"].max()), 4)])), flush=True)


if __name__ == "__main__":
    main()
