"""Timing of the stabiliser's occlusion test at 1280x720 ("Occlusion test"), one process, HIP events on the context's
stream, medians over repeated, warmed-up calls:

  (a) one rsdsfm_stabilize_window_frame_dev against (b) one rsdsfm_stabilize_visible_frame_dev through a window of 90 % of the frame, BGR,
      with the source plane and the counters, on one solved pair of a render_sequence clip with a share --holes of its depth map zeroed at
      random, onto an EMPTY mask; (c) and (d) the same two onto a mask that is 90 % set (the own frame's share in a stabilised clip is
      higher still).  The in-out planes are restored before every timed call, outside the timed window; the four alternate, so that all see
      the same machine;
  (e) the contended splat: (b) with the virtual camera 30 units behind the scene (m = (0, 0, 30)), so that every source pixel lands on a small
      patch of the z-buffer, against (f) the window call with that pose;
  (g) rsdsfm_stabilize_video_blended_dev with occlusion 0 against (h) with occlusion 1 at radius 2 over 16 pairs at B = 8, alternating, per
      pair, with the spread of the repetitions.
The expectations from bytes only: the map pass moves 8 B more per pixel on its 16 (zv written, the z-buffer reset and
splatted), the warp pass is unchanged where the mask is set and reads 4 + 9 more values per pixel that is still empty and valid.  No time is
gated.  Every line says what came out.  One JSON line per measurement; the record is profiles/stabilize_visible_time.txt.

    python tools/stabilize_visible_time.py [--reps 20] [--clip-reps 5] [--warmup 3] [--holes 0.33] > profiles/stabilize_visible_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stabilize_time import BATCH, COLS, PAIRS, ROWS, clip  # noqa: E402  (the stabiliser's clip and sizes)

RADIUS = 2
FEATHER = 16


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
    far = np.array([0.0, 0.0, 30.0])
    window = (ROWS // 20, COLS // 20, (9 * ROWS) // 10, ((9 * ROWS) // 10 * COLS) // ROWS)

    def event_pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        d_a, d_b = torch.from_numpy(frames[0]).to(dev), torch.from_numpy(frames[1]).to(dev)
        flow = torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev)
        dm, R, t = (torch.zeros(n, dtype=torch.float64, device=dev) for n in (npix, ROWS * 9, ROWS * 3))
        out, mask, source = torch.empty_like(d_a), torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev), torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        s.deep_flow_dev(d_a.data_ptr(), d_b.data_ptr(), ROWS, COLS, 3, flow.data_ptr())
        s.solve_frame_dev(flow.data_ptr(), ROWS, COLS, K, 0.8, dm.data_ptr(), R.data_ptr(), t.data_ptr(), trials=50, tol=0.05)
        s.synchronize()
        torch.manual_seed(1)
        dm.mul_((torch.rand(npix, device=dev) >= args.holes).double())  # non-inliers carry no depth
        mask0 = torch.zeros((ROWS, COLS), dtype=torch.uint8, device=dev)
        mask90 = torch.ones((ROWS, COLS), dtype=torch.uint8, device=dev)
        mask90[:, :COLS // 10] = 0  # a band along one edge, as a stabilised frame leaves it
        image0 = d_b.clone()
        torch.cuda.synchronize()
        common = (d_a.data_ptr(), 3, dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, ROWS, COLS)
        tail = (window, out.data_ptr(), mask.data_ptr(), source.data_ptr(), counts.data_ptr())

        def restore(start):  # on the solver's stream (torch's current stream here), in front of the timed window
            out.copy_(image0), mask.copy_(start), source.copy_(start)

        wind = lambda pose: (lambda: s.stabilize_window_frame_dev(*common, pose[0], pose[1], 2, *tail))
        vis = lambda pose: (lambda: s.stabilize_visible_frame_dev(*common, pose[0], pose[1], 2, *tail))
        calls = dict(a=(mask0, wind((M, m))), b=(mask0, vis((M, m))), c=(mask90, wind((M, m))), d=(mask90, vis((M, m))), e=(mask0, vis((np.eye(3), far))),
                     f=(mask0, wind((np.eye(3), far))))
        for start, fn in calls.values():
            for _ in range(args.warmup):
                restore(start), fn()
        s.synchronize()
        ts, got = {k_: [] for k_ in calls}, {}
        for _ in range(args.reps):
            for name, (start, fn) in calls.items():
                restore(start)
                counts.zero_()
                e0, e1 = event_pair()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3)
                got[name] = counts.cpu().numpy().tolist()
        med = {k_: float(np.median(v_)) for k_, v_ in ts.items()}
        mm = lambda k_: [round(min(ts[k_]), 1), round(max(ts[k_]), 1)]
        print(json.dumps(dict(what="frame", size="%dx%d" % (COLS, ROWS), holes=args.holes, reps=args.reps, window=list(window),
                              launches=dict(window=rsdsfm.stabilize_window_launches(ROWS, COLS), visible=rsdsfm.stabilize_visible_launches(ROWS, COLS)),
                              a_window_mask0_us=round(med["a"], 1), a_min_max_us=mm("a"), b_visible_mask0_us=round(med["b"], 1), b_min_max_us=mm("b"),
                              b_minus_a_us=round(med["b"] - med["a"], 1), a_taken=got["a"][0], b_taken_rejected=got["b"],
                              c_window_mask90_us=round(med["c"], 1), c_min_max_us=mm("c"), d_visible_mask90_us=round(med["d"], 1), d_min_max_us=mm("d"),
                              d_minus_c_us=round(med["d"] - med["c"], 1), c_taken=got["c"][0], d_taken_rejected=got["d"])), flush=True)
        print(json.dumps(dict(what="contended splat", size="%dx%d" % (COLS, ROWS), reps=args.reps, pose="M = I, m = (0, 0, 30)",
                              f_window_us=round(med["f"], 1), f_min_max_us=mm("f"), e_visible_us=round(med["e"], 1), e_min_max_us=mm("e"),
                              e_minus_f_us=round(med["e"] - med["f"], 1), b_minus_a_us=round(med["b"] - med["a"], 1),
                              atomics_dominate=bool((med["e"] - med["f"]) > 2.0 * (med["b"] - med["a"])), e_taken_rejected=got["e"])), flush=True)
        # the clip: (g) and (h) alternate
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        mk = lambda shape, dt: [torch.empty(shape, dtype=dt, device=dev) for _ in range(PAIRS)]
        like = lambda: [torch.empty_like(d_frames[0]) for _ in range(PAIRS)]
        dms, flows, Rs, Ts = mk(npix, torch.float64), mk((ROWS, COLS, 2), torch.float64), mk(ROWS * 9, torch.float64), mk(ROWS * 3, torch.float64)
        stabs, smasks, sources = like(), mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        crops, cmasks, csources = like(), mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        blends, bmasks, bsources = like(), mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        p = lambda xs: [x.data_ptr() for x in xs]
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        head = (p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks), p(crops), p(cmasks), p(blends), p(bmasks), p(bsources))
        kw = dict(blend_feather=FEATHER, d_crop_sources=p(csources), max_empty=npix // 100, margin=1, d_sources=p(sources), fill_radius=RADIUS, trials=50, tol=0.05)
        plain = lambda: s.stabilize_video_blended_dev(*head, **kw)
        tested = lambda: s.stabilize_video_blended_dev(*head, occlusion=True, **kw)
        for _ in range(args.warmup):
            plain(), s.synchronize(), tested(), s.synchronize()
        tg, th_, res = [], [], {}
        for _ in range(args.clip_reps):
            for name, fn, acc in (("g", plain, tg), ("h", tested, th_)):
                e0, e1 = event_pair()
                e0.record(stream)
                res[name] = fn()
                s.synchronize()
                e1.record(stream)
                e1.synchronize()
                acc.append(e0.elapsed_time(e1) / PAIRS)
        g, h = float(np.median(tg)), float(np.median(th_))
        r = res["h"]
        renders = 3 * sum(len(rsdsfm.neighbour_poses(r["A"], r["c"], r["A_s"], r["c_s"], r["scales"], q, RADIUS)[0]) for q in range(PAIRS)) / PAIRS
        filled = lambda x: int(x["crop_counts"][:, 2:].sum())
        print(json.dumps(dict(what="clip", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, batch=BATCH, radius=RADIUS, feather=FEATHER, reps=args.clip_reps,
                              window=list(r["window"]), g_blended_occlusion0_ms_per_pair=round(g, 3), g_min_max_ms=[round(min(tg), 3), round(max(tg), 3)],
                              h_blended_occlusion1_ms_per_pair=round(h, 3), h_min_max_ms=[round(min(th_), 3), round(max(th_), 3)],
                              h_minus_g_us_per_pair=round((h - g) * 1e3, 1), neighbour_renders_per_pair=round(renders, 2),
                              h_minus_g_us_per_render=round((h - g) * 1e3 / renders, 1), h_minus_g_percent_of_g=round(100.0 * (h - g) / g, 2),
                              g_spread_percent=round(100.0 * (max(tg) - min(tg)) / g, 2), h_within_g_spread=bool((h - g) <= (max(tg) - min(tg))),
                              crop_filled_pixels=dict(occlusion0=filled(res["g"]), occlusion1=filled(r)),
                              crop_none_pixels=dict(occlusion0=int(res["g"]["crop_counts"][:, 0].sum()), occlusion1=int(r["crop_counts"][:, 0].sum())))), flush=True)


if __name__ == "__main__":
    main()
