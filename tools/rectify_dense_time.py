"""Timing of the dense global-shutter rectifier at 1280x720 ("Dense global-shutter frames"), one process, HIP events on the
context's stream, medians over repeated, warmed-up calls:

  (a) rsdsfm_rectify_frame_dev / rsdsfm_rectify_gray_frame_dev (the forward splat) and
  (b) rsdsfm_rectify_dense_frame_dev, BGR and gray, on one solved pair of a render_sequence clip, a share --holes of its depth map zeroed at random -- (b) also against the HBM floor of its own
      byte count (rectify_dense_kernels.hip: 34 B per BGR pixel, 30 B per gray one, at the 8.0 TB/s peak);
  (c) rsdsfm_solve_video_dev and (d) rsdsfm_rectify_dense_video_dev over 16 pairs at B = 8, alternating, per pair -- (d) - (c) against the
      spread of (c)'s repetitions.
One JSON line per measurement; the record is profiles/rectify_dense_time.txt.

    python tools/rectify_dense_time.py [--reps 20] [--clip-reps 7] [--warmup 3] [--holes 0.33] > profiles/rectify_dense_time.txt
    python tools/rectify_dense_time.py --once   # warm-up, then TEN dense BGR frames (for rocprofv3 --kernel-trace --stats)
    python tools/rectify_dense_time.py --reduce-trace DIR_OR_DB > profiles/rectify_dense_trace.txt   # no GPU: reduces the result database of
                                                   # rocprofv3 --kernel-trace --stats -d DIR -- python tools/rectify_dense_time.py --once
    python tools/rectify_dense_time.py --iterations-table > profiles/rectify_dense_iterations.txt   # no GPU: the fixed point's error per
                                                   # iteration count, from the committed spec (what the default of 3 rests on)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS, PAIRS, BATCH = 720, 1280, 16, 8
HBM_PEAK = 8.0e12  # bytes per second


def clip(rsdsfm, nframes):
    K = (0.75 * COLS, 0.75 * COLS, 0.5 * COLS, 0.5 * ROWS)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(ROWS, COLS, K, v, w, k, 0.8, _model_only=True)
    s = 5.0 / np.abs(f0).max()
    frames, _, _ = rsdsfm.synth.render_sequence(nframes, ROWS, COLS, K, v * s, w * s, k, 0.8, seed=1)
    return frames, K


def reduce_trace(path):
    """the dense rectifier's dispatches in rocprofv3's result database: the launches of one frame in order, per-kernel medians, and the
    span / busy time of the last ten frames"""
    import glob
    import sqlite3
    import statistics as st

    if os.path.isdir(path):
        path = sorted(glob.glob(os.path.join(path, "**", "*.db"), recursive=True))[0]
    db = sqlite3.connect(path)
    rows = list(db.execute("select name, start, end, duration, grid_x, grid_y, workgroup_x, workgroup_y from kernels where name like '%rectify_dense%' order by start"))
    short = lambda n: n.split("(")[0].replace("rsdsfm::", "")
    per_frame = 9  # at 1280x720 (rsdsfm_rectify_dense_launches)
    print("# rocprofv3 --kernel-trace --stats -- python tools/rectify_dense_time.py --once, reduced by tools/rectify_dense_time.py --reduce-trace")
    print("# (MI355X, dense BGR frames at 1280x720, 33 % of the depth map zeroed; times under the tracer, which slows the host: the span is not the untraced call time)")
    print("%d dispatches = %d frames of %d launches" % (len(rows), len(rows) // per_frame, per_frame))
    frames = [rows[len(rows) - (i + 1) * per_frame:len(rows) - i * per_frame] for i in range(10)][::-1]
    print("per frame (last 10): span median %.1f us, kernels busy median %.1f us" % (st.median(f[-1][2] - f[0][1] for f in frames) / 1e3,
                                                                                    st.median(sum(x[3] for x in f) for f in frames) / 1e3))
    print("one frame in order:")
    for n, _, _, d, gx, gy, wx, wy in frames[5]:
        print("  %-34s grid %6d x %-4d block %4d x %d  %6.1f us" % (short(n), gx, gy, wx, wy, d / 1e3))
    per = {}
    for n, _, _, d, *_ in rows:
        per.setdefault(short(n), []).append(d)
    for n, v in per.items():
        print("%-34s n = %3d  median %.2f us" % (n, len(v), st.median(v) / 1e3))


def iterations_table():
    """tests/rectify_dense_spec_numpy.py at 96 x 128 on synth.scene_depth (the setup of tests/test_rectify_dense_cpu.py's accuracy test, at its
    motion and at 3.5 x it; no holes, 30 % and 60 % random holes with a 12 x 20 block): position error in the interior band after n
    iterations against the 60-step fixed point of the SAME displacement plane and against the 80-step inverse of the float64 map on the
    TRUE depth, and the mean abs error of the 3-iteration image against the texture at that true inverse"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    sys.path.insert(0, os.path.join(root, "oracle"))
    import oracle_py
    import rectify_dense_spec_numpy as spec

    import rsdsfm

    synth = rsdsfm.synth
    rows, cols, seed = 96, 128, 0x5EED0000
    K = (0.8 * cols, 0.8 * cols, cols / 2.0 - 0.3, rows / 2.0 + 0.2)
    depth = synth.scene_depth(rows, cols)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    frame = np.rint(synth._texture(xx, yy, seed)).astype(np.uint8)
    for scale in (1.0, 3.5):
        R, t = oracle_py.pose_table(scale * np.array([0.03, 0.03, 0.0]), scale * np.array([0.02, -0.03, 0.125]), 0.1, 0.8, rows)
        R = R.reshape(rows, 9)
        gx, gy, _ = spec.forward_map(depth, R, t, *K)
        F = np.stack([gx - xx, gy - yy], axis=-1)
        px, py = xx.copy(), yy.copy()
        for _ in range(80):
            d = synth._bilinear(F, px, py)
            px, py = xx - d[..., 0], yy - d[..., 1]
        truth = synth._texture(px, py, seed)
        band = int(np.ceil(np.abs(F).max())) + 3
        inner = np.zeros((rows, cols), dtype=bool)
        inner[band:rows - band, band:cols - band] = True
        for holes in (0.0, 0.3, 0.6):
            rng = np.random.default_rng(7)
            h = depth.copy()
            h[rng.random(h.shape) < holes] = 0.0
            if holes:
                h[40:52, 50:70] = 0.0
            out = spec.rectify_dense(frame, h, R, t, *K, iterations=3)
            ex, ey = spec.inverse_positions(out["disp"], 60)
            rec = dict(motion_scale=scale, holes=holes, max_displacement_per_axis_px=round(float(np.abs(F).max()), 2),
                       max_displacement_norm_px=round(float(np.hypot(F[..., 0], F[..., 1]).max()), 2), band=band,
                       mean_abs_error_3_iterations=round(float(np.abs(out["image"].astype(np.float64) - truth)[inner].mean()), 4),
                       mask_all_one_in_band=bool(out["mask"][inner].all()))
            for it in (1, 2, 3, 4, 6):
                qx, qy = spec.inverse_positions(out["disp"], it)
                rec["it%d_px_vs_fixed_point" % it] = round(float(np.hypot(qx - ex, qy - ey)[inner].max()), 4)
                rec["it%d_px_vs_true_depth_inverse" % it] = round(float(np.hypot(qx - px, qy - py)[inner].max()), 4)
            print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--clip-reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--holes", type=float, default=0.33, help="share of the solved depth map zeroed at random for (a) and (b): the synthetic pair keeps every pixel")
    ap.add_argument("--once", action="store_true", help="warm-up, then TEN dense BGR frames and nothing else (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--reduce-trace", default=None, metavar="DIR_OR_DB", help="no GPU: reduce rocprofv3's result database of a --once run")
    ap.add_argument("--iterations-table", action="store_true", help="no GPU: the fixed point's error per iteration count, from the spec")
    args = ap.parse_args()
    if args.reduce_trace:
        return reduce_trace(args.reduce_trace)
    if args.iterations_table:
        return iterations_table()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    frames, K = clip(rsdsfm, PAIRS + 1)
    gray = [np.ascontiguousarray(f[:, :, 1]) for f in frames]
    npix = ROWS * COLS

    def timed(s, fn, reps):
        """median and spread (ms) of fn() between two events on the context's stream"""
        for _ in range(args.warmup):
            fn()
        s.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    with torch.cuda.device(dev), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        for name, fr, ch in (("bgr", frames, 3), ("gray", gray, 1)):
            d_a, d_b = torch.from_numpy(fr[0]).to(dev), torch.from_numpy(fr[1]).to(dev)
            flow = torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev)
            dm, R, t = (torch.zeros(n, dtype=torch.float64, device=dev) for n in (npix, ROWS * 9, ROWS * 3))
            prev = torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
            gs, fixed, dense = torch.empty_like(d_a), torch.empty_like(d_a), torch.empty_like(d_a)
            mask = torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
            c3 = torch.empty((ROWS, COLS, 3), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            s.deep_flow_dev(d_a.data_ptr(), d_b.data_ptr(), ROWS, COLS, ch, flow.data_ptr())
            r = s.solve_frame_dev(flow.data_ptr(), ROWS, COLS, K, 0.8, dm.data_ptr(), R.data_ptr(), t.data_ptr(), trials=50, tol=0.05)
            s.synchronize()
            torch.manual_seed(1)
            dm.mul_((torch.rand(npix, device=dev) >= args.holes).double())  # non-inliers carry no depth
            holes = float((dm == 0).double().mean())
            torch.cuda.synchronize()
            splat_fn = s.rectify_gray_frame_dev if ch == 1 else s.rectify_frame_dev
            splat = lambda: splat_fn(r["d_inliers"], r["num_inliers"], d_a.data_ptr(), dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, ROWS, COLS, prev.data_ptr(),
                                     gs.data_ptr(), fixed.data_ptr(), c3.data_ptr(), offset=1)
            dns = lambda: s.rectify_dense_frame_dev(d_a.data_ptr(), ch, dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, ROWS, COLS, dense.data_ptr(), mask.data_ptr())
            if args.once:
                for _ in range(args.warmup + 10):
                    dns()
                s.synchronize()
                print(json.dumps(dict(what="once", image=name, frames=10, warmup=args.warmup, launches_per_frame=rsdsfm.rectify_dense_launches(ROWS, COLS))))  # 9: pull to level 1, 2 pulls, the single workgroup, 3 pushes, map, warp
                return
            a = timed(s, splat, args.reps)
            b = timed(s, dns, args.reps)
            floor_us = (30 + 4 * (ch == 3)) * npix / HBM_PEAK * 1e6
            print(json.dumps(dict(what="frame", image=name, size="%dx%d" % (COLS, ROWS), inliers=int(r["num_inliers"]), holes=round(holes, 3),
                                  a_splat_us=round(a[0] * 1e3, 1), b_dense_us=round(b[0] * 1e3, 1), b_min_max_us=[round(b[1] * 1e3, 1), round(b[2] * 1e3, 1)],
                                  b_over_a=round(b[0] / a[0], 2), b_hbm_floor_us=round(floor_us, 1), b_over_floor=round(b[0] * 1e3 / floor_us, 1),
                                  covered_by_splat=round(float((gs.reshape(ROWS, COLS, -1) != 0).any(dim=2).double().mean()), 3),
                                  covered_by_dense=round(float(mask.double().mean()), 3))), flush=True)
        # the clip: (c) and (d) alternate, so that both see the same machine
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        dms = [torch.empty(npix, dtype=torch.float64, device=dev) for _ in range(PAIRS)]
        denses = [torch.empty_like(d_frames[0]) for _ in range(PAIRS)]
        fp, mp, op = [x.data_ptr() for x in d_frames], [x.data_ptr() for x in dms], [x.data_ptr() for x in denses]
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        solve = lambda: s.solve_video_dev(fp, ROWS, COLS, 3, K, 0.8, mp, trials=50, tol=0.05)
        both = lambda: s.rectify_dense_video_dev(fp, ROWS, COLS, 3, K, 0.8, mp, op, trials=50, tol=0.05)
        for _ in range(args.warmup):
            solve(), s.synchronize(), both()
        tc, td = [], []
        for _ in range(args.clip_reps):
            for fn, acc in ((solve, tc), (both, td)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                s.synchronize()  # (solve_video_dev returns with its lanes still running)
                e1.record(stream)
                e1.synchronize()
                acc.append(e0.elapsed_time(e1) / PAIRS)
        c, d = float(np.median(tc)), float(np.median(td))
        print(json.dumps(dict(what="clip", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, batch=BATCH, c_solve_video_ms_per_pair=round(c, 3),
                              c_min_max_ms=[round(min(tc), 3), round(max(tc), 3)], d_dense_video_ms_per_pair=round(d, 3), d_min_max_ms=[round(min(td), 3), round(max(td), 3)],
                              d_minus_c_us_per_pair=round((d - c) * 1e3, 1), d_minus_c_percent_of_c=round(100.0 * (d - c) / c, 2),
                              c_spread_percent=round(100.0 * (max(tc) - min(tc)) / c, 2))), flush=True)


if __name__ == "__main__":
    main()
