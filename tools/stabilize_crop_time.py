"""Timing of the stabiliser's crop and zoom at 1280x720 ("Crop and zoom"), one process, HIP events on the context's
stream, medians over repeated, warmed-up calls:

  (a) rsdsfm_crop_window_dev on 16 masks (a band of about 5 % of each side empty along two edges, shifted from mask to mask, as stabilised
      frames leave it), margin 1: the three launches, the 8-byte copy and the wait;
  (b) one rsdsfm_stabilize_fill_frame_dev on an empty mask against (c) one rsdsfm_stabilize_window_frame_dev on a zeroed mask through a
      window of 90 % of the frame, BGR, with the source plane and the counter, on one solved pair of a render_sequence clip with a share
      --holes of its depth map zeroed at random.  The in-out planes are restored before every timed call, outside the timed window;
      (a), (b) and (c) alternate, so that all see the same machine;
  (d) rsdsfm_stabilize_video_filled_dev against (e) rsdsfm_stabilize_video_cropped_dev at radius 2 over 16 pairs at B = 8, alternating, per
      pair, with the spread of the repetitions.
The expectations: (c) costs what (b) costs -- the extra work per pixel is two multiply-adds --, (e) - (d) is roughly one
more set of passes per pair (the own frame and its neighbours through the window) plus the search; the search's cost was not known.  Every
line says what came out.  One JSON line per measurement; the record is profiles/stabilize_crop_time.txt.

    python tools/stabilize_crop_time.py [--reps 20] [--clip-reps 5] [--warmup 3] [--holes 0.33] > profiles/stabilize_crop_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

RADIUS = 2
MASKS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clip-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--holes", type=float, default=0.33, help="share of the solved depth map zeroed at random: the synthetic pair keeps every pixel")
    args = ap.parse_args()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    frames, K = clip(rsdsfm, PAIRS + 1)
    npix = ROWS * COLS
    axis = np.array([0.005, -0.006, 0.004])  # tools/stabilize_fill_time.py's pose
    th = np.linalg.norm(axis)
    X = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    M = np.eye(3) + np.sin(th) / th * X + (1.0 - np.cos(th)) / th ** 2 * (X @ X)
    m = np.array([0.01, -0.008, 0.004])
    window = (ROWS // 20, COLS // 20, (9 * ROWS) // 10, ((9 * ROWS) // 10 * COLS) // ROWS)

    def event_pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        d_a, d_b = torch.from_numpy(frames[0]).to(dev), torch.from_numpy(frames[1]).to(dev)
        flow = torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev)
        dm, R, t = (torch.zeros(n, dtype=torch.float64, device=dev) for n in (npix, ROWS * 9, ROWS * 3))
        out, mask, source = torch.empty_like(d_a), torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev), torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        filled = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        s.deep_flow_dev(d_a.data_ptr(), d_b.data_ptr(), ROWS, COLS, 3, flow.data_ptr())
        s.solve_frame_dev(flow.data_ptr(), ROWS, COLS, K, 0.8, dm.data_ptr(), R.data_ptr(), t.data_ptr(), trials=50, tol=0.05)
        s.synchronize()
        torch.manual_seed(1)
        dm.mul_((torch.rand(npix, device=dev) >= args.holes).double())  # non-inliers carry no depth
        band_r, band_c = int(round(0.0513 * ROWS)), int(round(0.0513 * COLS))
        planes = []
        for k in range(MASKS):  # the band wanders by up to 15 pixels
            pm = torch.ones((ROWS, COLS), dtype=torch.uint8, device=dev)
            pm[:band_r + (k * 7) % 16, :] = 0
            pm[:, :band_c + (k * 5) % 16] = 0
            planes.append(pm)
        mask0 = torch.zeros((ROWS, COLS), dtype=torch.uint8, device=dev)
        image0 = d_b.clone()
        torch.cuda.synchronize()
        common = (d_a.data_ptr(), 3, dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, ROWS, COLS)
        found = {}

        def restore(start):  # on the solver's stream (torch's current stream here), in front of the timed window
            if start is not None:
                out.copy_(image0), mask.copy_(start), source.copy_(start)

        def search():
            found["w"] = s.crop_window_dev([pm.data_ptr() for pm in planes], ROWS, COLS, 0, 1)

        fill = lambda: s.stabilize_fill_frame_dev(*common, M, m, 2, out.data_ptr(), mask.data_ptr(), source.data_ptr(), filled.data_ptr())
        wind = lambda: s.stabilize_window_frame_dev(*common, M, m, 2, window, out.data_ptr(), mask.data_ptr(), source.data_ptr(), filled.data_ptr())
        calls = dict(a=(None, search), b=(mask0, fill), c=(mask0, wind))
        for start, fn in calls.values():
            for _ in range(args.warmup):
                restore(start), fn()
        s.synchronize()
        ts, taken = dict(a=[], b=[], c=[]), {}
        for _ in range(args.reps):
            for name, (start, fn) in calls.items():
                restore(start)
                e0, e1 = event_pair()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3)
                taken[name] = int(filled.cpu())
        med = {k_: float(np.median(v_)) for k_, v_ in ts.items()}
        mm = lambda k_: [round(min(ts[k_]), 1), round(max(ts[k_]), 1)]
        print(json.dumps(dict(what="window", size="%dx%d" % (COLS, ROWS), masks=MASKS, margin=1, reps=args.reps, launches=rsdsfm.crop_window_launches(ROWS, COLS),
                              a_crop_window_us=round(med["a"], 1), a_min_max_us=mm("a"), window=list(found["w"]))), flush=True)
        print(json.dumps(dict(what="frame", size="%dx%d" % (COLS, ROWS), holes=args.holes, reps=args.reps, window=list(window),
                              launches=dict(b=rsdsfm.stabilize_fill_launches(ROWS, COLS), c=rsdsfm.stabilize_window_launches(ROWS, COLS)),
                              b_fill_mask0_us=round(med["b"], 1), b_min_max_us=mm("b"), c_window_mask0_us=round(med["c"], 1), c_min_max_us=mm("c"),
                              b_taken=taken["b"], c_taken=taken["c"], c_minus_b_us=round(med["c"] - med["b"], 1),
                              c_within_b_spread=bool(abs(med["c"] - med["b"]) <= max(ts["b"]) - min(ts["b"])))), flush=True)
        # the clip: (d) and (e) alternate
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        mk = lambda shape, dt: [torch.empty(shape, dtype=dt, device=dev) for _ in range(PAIRS)]
        dms, flows, Rs, Ts = mk(npix, torch.float64), mk((ROWS, COLS, 2), torch.float64), mk(ROWS * 9, torch.float64), mk(ROWS * 3, torch.float64)
        stabs, smasks, sources = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        crops, cmasks, csources = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)], mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        p = lambda xs: [x.data_ptr() for x in xs]
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        head = (p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks))
        fillv = lambda: s.stabilize_video_filled_dev(*head, p(sources), fill_radius=RADIUS, trials=50, tol=0.05)
        cropv = lambda: s.stabilize_video_cropped_dev(*head, p(crops), p(cmasks), p(csources), max_empty=npix // 100, margin=1, d_sources=p(sources), fill_radius=RADIUS,
                                                      trials=50, tol=0.05)
        for _ in range(args.warmup):
            fillv(), s.synchronize(), cropv(), s.synchronize()
        td, te = [], []
        res = None
        for _ in range(args.clip_reps):
            for fn, acc in ((fillv, td), (cropv, te)):
                e0, e1 = event_pair()
                e0.record(stream)
                res = fn()
                s.synchronize()
                e1.record(stream)
                e1.synchronize()
                acc.append(e0.elapsed_time(e1) / PAIRS)
        d, e = float(np.median(td)), float(np.median(te))
        passes = 1 + sum(len(rsdsfm.neighbour_poses(res["A"], res["c"], res["A_s"], res["c_s"], res["scales"], q, RADIUS)[0]) for q in range(PAIRS)) / PAIRS
        cc = res["crop_counts"]
        print(json.dumps(dict(what="clip", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, batch=BATCH, radius=RADIUS, reps=args.clip_reps, max_empty=npix // 100, margin=1,
                              window=list(res["window"]), d_filled_video_ms_per_pair=round(d, 3), d_min_max_ms=[round(min(td), 3), round(max(td), 3)],
                              e_cropped_video_ms_per_pair=round(e, 3), e_min_max_ms=[round(min(te), 3), round(max(te), 3)],
                              e_minus_d_us_per_pair=round((e - d) * 1e3, 1), window_passes_per_pair=round(passes, 2),
                              e_minus_d_us_per_pass=round((e - d) * 1e3 / passes, 1), e_minus_d_percent_of_d=round(100.0 * (e - d) / d, 2),
                              d_spread_percent=round(100.0 * (max(td) - min(td)) / d, 2), e_within_d_spread=bool((e - d) <= (max(td) - min(td))),
                              crop_own_mean_share=round(float(cc[:, 1].mean()) / npix, 4), crop_filled_mean_share=round(float(cc[:, 2:].sum(axis=1).mean()) / npix, 4),
                              crop_none_mean_share=round(float(cc[:, 0].mean()) / npix, 4))), flush=True)


if __name__ == "__main__":
    main()
