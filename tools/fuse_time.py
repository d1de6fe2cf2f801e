"""Timing of the depth fusion at 1280x720 ("Depth fusion"), one process, HIP events on the context's stream, medians over
repeated, warmed-up calls, the variants of one comparison alternating:

  (1) rsdsfm_fuse_depths_dev over 16 pairs (15 links) in one call -- with the records (one copy and a wait at the end) and enqueue-only --
      against the HBM floor of the bytes it moves (fuse_kernels.hip: per pixel and link 8 B preset + 8 B depth + 16 B field for the splat;
      per pixel and pair 8 B own depth read, 8 B fused + 1 B flags written, and per pixel and link 8 B splat word + 16 B field + 8 B gathered
      for the merge; at the 8.0 TB/s peak).  The maps are synthetic (a smooth scene, 60 % of the pixels with a depth, as a solve with
      outliers leaves them), the records are rsdsfm_link_pairs_dev's on them;
  (2) rsdsfm_solve_video_linked_dev over 16 pairs at B = 8 without and with d_fused (Solver.solve_video_linked_dev), per pair, with the
      spread of each one's repetitions.  The statement to confirm or refute: the added cost per pair lies inside the repetition spread of
      the linked clip call without fusion, measured in the same run.
One JSON line per measurement; the record is profiles/fuse_time.txt.

    python tools/fuse_time.py [--reps 20] [--clip-reps 5] [--warmup 2] > profiles/fuse_time.txt
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
        # (1) the fusion alone
        r = np.random.default_rng(1)
        field = torch.from_numpy(np.ascontiguousarray(f0 * sc)).to(dev)
        Z = rsdsfm.synth.scene_depth(ROWS, COLS)
        maps = []
        for q in range(PAIRS):
            z = Z * (1.0 + 0.1 * q) * np.exp(r.normal(0.0, 0.02, (ROWS, COLS)))
            z[r.uniform(size=(ROWS, COLS)) < 0.4] = 0.0
            maps.append(torch.from_numpy(np.ascontiguousarray(z.T)).to(dev))
        fused = [torch.empty(npix, dtype=torch.float64, device=dev) for _ in range(PAIRS)]
        flags = [torch.empty(npix, dtype=torch.uint8, device=dev) for _ in range(PAIRS)]
        torch.cuda.synchronize()
        ptrs = lambda a: [t.data_ptr() for t in a]
        fp, mp, up, gp = [field.data_ptr()] * PAIRS, ptrs(maps), ptrs(fused), ptrs(flags)
        vs, ws, ks = [v / np.linalg.norm(v)] * PAIRS, [w] * PAIRS, [0.0] * PAIRS
        links = s.link_pairs_dev(fp, mp, vs, ws, ks, ROWS, COLS, K, 0.8)
        res = {}
        fuse = lambda rec: (lambda: res.__setitem__(rec, s.fuse_depths_dev(fp, mp, vs, ws, ks, ROWS, COLS, K, 0.8, links, up, d_flags=gp, want_records=rec)))
        t_rec, t_enq = alternating(s, [fuse(True), fuse(False)], args.reps)
        nl = PAIRS - 1
        total_bytes = npix * (nl * (8 + 8 + 16) + PAIRS * (8 + 8 + 1) + nl * (8 + 16 + 8))
        floor_us = total_bytes / HBM_PEAK * 1e6
        rec = res[True]
        holes = sum(npix - x["own"] for x in rec)
        for what, t in (("fusion, records", t_rec), ("fusion, enqueue only", t_enq)):
            print(json.dumps(dict(what=what, size="%dx%d" % (COLS, ROWS), pairs=PAIRS, links=nl, launches=3, us=round(t[0] * 1e3, 1),
                                  min_max_us=[round(t[1] * 1e3, 1), round(t[2] * 1e3, 1)], us_per_pair=round(t[0] * 1e3 / PAIRS, 1),
                                  bytes_per_pixel_and_pair=round(total_bytes / npix / PAIRS, 1), hbm_floor_us=round(floor_us, 1),
                                  over_floor=round(t[0] * 1e3 / floor_us, 2), usable_links=sum(1 for x in links if x["valid"] and x["ratio"] > 0),
                                  holes_filled_share=round(sum(x["filled_prev"] + x["filled_next"] for x in rec) / max(holes, 1), 4),
                                  confirmed_share=round(sum(x["confirmed"] for x in rec) / max(sum(x["own"] for x in rec), 1), 4))), flush=True)
        del maps, fused, flags
        # (2) the clip
        frames, _, _ = rsdsfm.synth.render_sequence(PAIRS + 1, ROWS, COLS, K, v, w, k, 0.8, seed=1)
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        dms = [torch.empty(npix, dtype=torch.float64, device=dev) for _ in range(PAIRS)]
        fields = [torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev) for _ in range(PAIRS)]
        fused = [torch.empty(npix, dtype=torch.float64, device=dev) for _ in range(PAIRS)]
        flags = [torch.empty(npix, dtype=torch.uint8, device=dev) for _ in range(PAIRS)]
        fr, mp, fl, up, gp = ptrs(d_frames), ptrs(dms), ptrs(fields), ptrs(fused), ptrs(flags)
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        linked = lambda: res.__setitem__("linked", s.solve_video_linked_dev(fr, ROWS, COLS, 3, K, 0.8, mp, fl, trials=50, tol=0.05))
        with_fusion = lambda: res.__setitem__("fused", s.solve_video_linked_dev(fr, ROWS, COLS, 3, K, 0.8, mp, fl, trials=50, tol=0.05, d_fused=up, d_flags=gp))
        c, d = alternating(s, [linked, with_fusion], args.clip_reps, wait=True)
        fu = res["fused"]["fuse"]
        print(json.dumps(dict(what="clip", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, batch=BATCH, linked_ms_per_pair=round(c[0] / PAIRS, 3),
                              linked_min_max_ms=[round(c[1] / PAIRS, 3), round(c[2] / PAIRS, 3)], linked_spread_percent=round(100.0 * (c[2] - c[1]) / c[0], 2),
                              fused_ms_per_pair=round(d[0] / PAIRS, 3), fused_min_max_ms=[round(d[1] / PAIRS, 3), round(d[2] / PAIRS, 3)],
                              fused_spread_percent=round(100.0 * (d[2] - d[1]) / d[0], 2), fused_over_linked=round(d[0] / c[0], 4),
                              fused_minus_linked_us_per_pair=round((d[0] - c[0]) / PAIRS * 1e3, 1), added_cost_inside_linked_spread=bool(d[0] - c[0] <= c[2] - c[1]),
                              own=sum(x["own"] for x in fu), filled=sum(x["filled_prev"] + x["filled_next"] for x in fu), left=sum(x["left"] for x in fu))), flush=True)


if __name__ == "__main__":
    main()
