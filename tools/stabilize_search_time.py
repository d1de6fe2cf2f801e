"""Timing of the stabiliser's search for the visible pre-image at 1280x720 ("Visible pre-image"), one process, HIP events on
the context's stream, medians over repeated, warmed-up calls (tools/stabilize_visible_time.py's protocol):

  (a) one rsdsfm_stabilize_visible_frame_dev against (b) one rsdsfm_stabilize_search_frame_dev through a window of 90 % of the frame, BGR,
      with the source plane and the counters, on one solved pair of a render_sequence clip with a share --holes of its depth map zeroed at
      random, onto an EMPTY mask; (c) and (d) the same two onto a mask that is 90 % set.  The in-out planes are restored before every timed
      call, outside the timed window; the variants alternate, so that all see the same machine;
  (e) and (f) the same two on the FOLD scene of tests/stabilize_visible_cases.py scaled to the frame (a box at depth 2 over a background at
      depth 10, identity pose tables, the virtual camera moved sideways by 0.6: a fold band of 0.24 cols), onto an empty mask, so that the
      restart actually runs;
  (g) rsdsfm_stabilize_video_blended_dev with occlusion 1 and the knob (rsdsfm_set_occlusion_search) at 0 against (h) at 1, radius 2 over 16
      pairs at B = 8, alternating, per pair, with the spread of the repetitions.
The expectations from bytes only: the key plane doubles the z-buffer's bytes (8 B reset and at most one 8-byte atomic per
pixel in the map pass instead of 4), the 3 x 3 read of an empty valid pixel grows from 36 B to 72 B, and a pixel that fails the test pays the
fixed point, 4 values of zv and the sample a second time.  No time is gated.  Every line says what came out.  One JSON line per measurement;
the record is profiles/stabilize_search_time.txt.

    python tools/stabilize_search_time.py [--reps 20] [--clip-reps 5] [--warmup 3] [--holes 0.33] > profiles/stabilize_search_time.txt
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


def fold_scene(rows, cols, seed=7):
    """tests/stabilize_visible_cases.fold_case's scene at this size: (image, depth, R, t, K, M, m)"""
    rng = np.random.default_rng(seed)
    r0, r1, c0, c1 = rows // 4, rows - rows // 4, (3 * cols) // 10 + cols // 8, (7 * cols) // 10 + cols // 8  # moved right: its footprint stays in the frame
    image = rng.integers(0, 96, size=(rows, cols, 3), dtype=np.uint8)
    image[r0:r1, c0:c1] = rng.integers(160, 256, size=(r1 - r0, c1 - c0, 3), dtype=np.uint8)
    depth = np.full((rows, cols), 10.0)
    depth[r0:r1, c0:c1] = 2.0
    R, t = np.tile(np.eye(3).reshape(1, 9), (rows, 1)), np.zeros((rows, 3))
    return image, depth, R, t, (float(cols), float(cols), cols / 2.0, rows / 2.0), np.eye(3), np.array([-0.6, 0.0, 0.0])


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
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_a, d_b = up(frames[0]), up(frames[1])
        flow = torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev)
        dm, R, t = (torch.zeros(n, dtype=torch.float64, device=dev) for n in (npix, ROWS * 9, ROWS * 3))
        out, mask, source = torch.empty_like(d_a), torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev), torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        counts = torch.zeros(3, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        s.deep_flow_dev(d_a.data_ptr(), d_b.data_ptr(), ROWS, COLS, 3, flow.data_ptr())
        s.solve_frame_dev(flow.data_ptr(), ROWS, COLS, K, 0.8, dm.data_ptr(), R.data_ptr(), t.data_ptr(), trials=50, tol=0.05)
        s.synchronize()
        torch.manual_seed(1)
        dm.mul_((torch.rand(npix, device=dev) >= args.holes).double())  # non-inliers carry no depth
        f_image, f_depth, f_R, f_t, f_K, f_M, f_m = fold_scene(ROWS, COLS)
        d_f, d_fdm, d_fR, d_ft = up(f_image), up(f_depth.T), up(f_R), up(f_t)
        mask0 = torch.zeros((ROWS, COLS), dtype=torch.uint8, device=dev)
        mask90 = torch.ones((ROWS, COLS), dtype=torch.uint8, device=dev)
        mask90[:, :COLS // 10] = 0  # a band along one edge, as a stabilised frame leaves it
        image0 = d_b.clone()
        torch.cuda.synchronize()
        solved = (d_a.data_ptr(), 3, dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, ROWS, COLS, M, m, 2, window)
        fold = (d_f.data_ptr(), 3, d_fdm.data_ptr(), d_fR.data_ptr(), d_ft.data_ptr(), f_K, ROWS, COLS, f_M, f_m, 2, (0, 0, ROWS, COLS))
        tail = (out.data_ptr(), mask.data_ptr(), source.data_ptr(), counts.data_ptr())

        def restore(start):  # on the solver's stream (torch's current stream here), in front of the timed window
            out.copy_(image0), mask.copy_(start), source.copy_(start)

        vis = lambda head: (lambda: s.stabilize_visible_frame_dev(*head, *tail))
        sea = lambda head: (lambda: s.stabilize_search_frame_dev(*head, *tail))
        calls = dict(a=(mask0, vis(solved)), b=(mask0, sea(solved)), c=(mask90, vis(solved)), d=(mask90, sea(solved)), e=(mask0, vis(fold)), f=(mask0, sea(fold)))
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
        for what, v, w in (("frame, empty mask", "a", "b"), ("frame, mask 90 % set", "c", "d"), ("fold scene, empty mask", "e", "f")):
            print(json.dumps(dict(what=what, size="%dx%d" % (COLS, ROWS), holes=args.holes if v != "e" else 0.0, reps=args.reps,
                                  launches=dict(visible=rsdsfm.stabilize_visible_launches(ROWS, COLS), search=rsdsfm.stabilize_search_launches(ROWS, COLS)),
                                  visible_us=round(med[v], 1), visible_min_max_us=mm(v), search_us=round(med[w], 1), search_min_max_us=mm(w),
                                  search_minus_visible_us=round(med[w] - med[v], 1), percent_of_visible=round(100.0 * (med[w] - med[v]) / med[v], 2),
                                  visible_spread_us=round(max(ts[v]) - min(ts[v]), 1), visible_taken_rejected=got[v][:2], search_taken_rejected_recovered=got[w])),
                  flush=True)
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
        kw = dict(blend_feather=FEATHER, d_crop_sources=p(csources), max_empty=npix // 100, margin=1, d_sources=p(sources), fill_radius=RADIUS, trials=50, tol=0.05,
                  occlusion=True)
        tested = lambda: s.stabilize_video_blended_dev(*head, **kw)
        searched = lambda: s.stabilize_video_blended_dev(*head, occlusion_search=True, **kw)
        for _ in range(args.warmup):
            tested(), s.synchronize(), searched(), s.synchronize()
        tg, th_, res = [], [], {}
        for _ in range(args.clip_reps):
            for name, fn, acc in (("g", tested, tg), ("h", searched, th_)):
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
                              window=list(r["window"]), g_blended_knob0_ms_per_pair=round(g, 3), g_min_max_ms=[round(min(tg), 3), round(max(tg), 3)],
                              h_blended_knob1_ms_per_pair=round(h, 3), h_min_max_ms=[round(min(th_), 3), round(max(th_), 3)],
                              h_minus_g_us_per_pair=round((h - g) * 1e3, 1), neighbour_renders_per_pair=round(renders, 2),
                              h_minus_g_us_per_render=round((h - g) * 1e3 / renders, 1), h_minus_g_percent_of_g=round(100.0 * (h - g) / g, 2),
                              g_spread_percent=round(100.0 * (max(tg) - min(tg)) / g, 2), h_within_g_spread=bool((h - g) <= (max(tg) - min(tg))),
                              crop_filled_pixels=dict(knob0=filled(res["g"]), knob1=filled(r)),
                              crop_none_pixels=dict(knob0=int(res["g"]["crop_counts"][:, 0].sum()), knob1=int(r["crop_counts"][:, 0].sum())))), flush=True)


if __name__ == "__main__":
    main()
