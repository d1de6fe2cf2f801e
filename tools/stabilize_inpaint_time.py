"""Timing of the stabiliser's inpainting at 1280x720 ("Inpaint"), one process, HIP events on the context's stream, medians
over repeated, warmed-up calls:

  (a) rsdsfm_inpaint_frame_dev, BGR, with the source plane and the counter, on the blend test's mask (99 % set: a band of 0.5 % of each
      side empty along two edges),
  (b) on a mask that is 67 % set (a third of the pixels empty at random) and
  (c) on an all-set mask (nothing to write: the pyramid and one mask byte per pixel), beside
  (d) rsdsfm_rectify_dense_frame_dev, BGR, on one solved pair with a third of its depth map zeroed at random: the call whose stage A this
      pyramid mirrors.  The in-out planes are restored before every timed call, outside the timed window; (a) .. (d) alternate, so that all
      see the same machine;
  (e) rsdsfm_stabilize_video_blended_dev against (f) rsdsfm_stabilize_video_inpainted_dev at radius 2 over 16 pairs at B = 8, alternating, per
      pair, with the spread of the repetitions.
The expectation: about 8 - 10 B per pixel of traffic, far below what the launches cost, so (a) .. (c) are launch-bound
at roughly the cost of the dense call's stage A, and (f) - (e) is two device copies and one such call per pair.  Every line says what came
out.  One JSON line per measurement; the record is profiles/stabilize_inpaint_time.txt.

    python tools/stabilize_inpaint_time.py [--reps 20] [--clip-reps 5] [--warmup 3] > profiles/stabilize_inpaint_time.txt
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
    args = ap.parse_args()
    import torch

    import rsdsfm

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    frames, K = clip(rsdsfm, PAIRS + 1)
    npix = ROWS * COLS

    def event_pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        own = torch.ones((ROWS, COLS), dtype=torch.uint8, device=dev)
        own[:max(int(round(0.005 * ROWS)), 1), :] = 0
        own[:, :max(int(round(0.005 * COLS)), 1)] = 0
        torch.manual_seed(1)
        third = (torch.rand((ROWS, COLS), device=dev) >= 0.33).to(torch.uint8)
        full = torch.ones_like(own)
        image0 = torch.from_numpy(frames[0]).to(dev)
        image, source = torch.empty_like(image0), torch.empty_like(own)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        # the dense call's inputs: one solved pair, a third of its map zeroed
        d_b = torch.from_numpy(frames[1]).to(dev)
        flow = torch.empty((ROWS, COLS, 2), dtype=torch.float64, device=dev)
        dm, R, t = (torch.zeros(n, dtype=torch.float64, device=dev) for n in (npix, ROWS * 9, ROWS * 3))
        dense, dmask = torch.empty_like(image0), torch.empty_like(own)
        torch.cuda.synchronize()
        s.deep_flow_dev(image0.data_ptr(), d_b.data_ptr(), ROWS, COLS, 3, flow.data_ptr())
        s.solve_frame_dev(flow.data_ptr(), ROWS, COLS, K, 0.8, dm.data_ptr(), R.data_ptr(), t.data_ptr(), trials=50, tol=0.05)
        s.synchronize()
        dm.mul_((torch.rand(npix, device=dev) >= 0.33).double())
        torch.cuda.synchronize()

        def restore(mask):  # on the solver's stream (torch's current stream here), in front of the timed window
            if mask is not None:
                image.copy_(image0), source.copy_(mask)

        inpaint = lambda mask: (lambda: s.inpaint_frame_dev(image.data_ptr(), mask.data_ptr(), 3, ROWS, COLS, source.data_ptr(), cnt.data_ptr()))
        calls = dict(a=(own, inpaint(own)), b=(third, inpaint(third)), c=(full, inpaint(full)),
                     d=(None, lambda: s.rectify_dense_frame_dev(image0.data_ptr(), 3, dm.data_ptr(), R.data_ptr(), t.data_ptr(), K, ROWS, COLS, dense.data_ptr(),
                                                                dmask.data_ptr())))
        for mask, fn in calls.values():
            for _ in range(args.warmup):
                restore(mask), fn()
        s.synchronize()
        ts, counts = {k_: [] for k_ in calls}, {}
        for _ in range(args.reps):
            for name, (mask, fn) in calls.items():
                restore(mask)
                e0, e1 = event_pair()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3)
                if mask is not None:
                    counts[name] = int(cnt.cpu()[0])
        med = {k_: float(np.median(v_)) for k_, v_ in ts.items()}
        mm = lambda k_: [round(min(ts[k_]), 1), round(max(ts[k_]), 1)]
        share = lambda m_: round(float(m_.sum().cpu()) / npix, 4)
        print(json.dumps(dict(what="frame", size="%dx%d" % (COLS, ROWS), reps=args.reps, set_share=dict(a=share(own), b=share(third), c=share(full)),
                              launches=dict(inpaint=rsdsfm.inpaint_launches(ROWS, COLS), dense=rsdsfm.rectify_dense_launches(ROWS, COLS)),
                              a_inpaint_own99_us=round(med["a"], 1), a_min_max_us=mm("a"), b_inpaint_set67_us=round(med["b"], 1), b_min_max_us=mm("b"),
                              c_inpaint_all_set_us=round(med["c"], 1), c_min_max_us=mm("c"), d_dense_us=round(med["d"], 1), d_min_max_us=mm("d"),
                              us_per_launch=dict(a=round(med["a"] / rsdsfm.inpaint_launches(ROWS, COLS), 2), d=round(med["d"] / rsdsfm.rectify_dense_launches(ROWS, COLS), 2)),
                              written=counts)), flush=True)
        # the clip: (e) and (f) alternate
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        mk = lambda shape, dt: [torch.empty(shape, dtype=dt, device=dev) for _ in range(PAIRS)]
        like = lambda: [torch.empty_like(d_frames[0]) for _ in range(PAIRS)]
        dms, flows, Rs, Ts = mk(npix, torch.float64), mk((ROWS, COLS, 2), torch.float64), mk(ROWS * 9, torch.float64), mk(ROWS * 3, torch.float64)
        stabs, smasks, sources = like(), mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        crops, cmasks, csources = like(), mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        blends, bmasks, bsources = like(), mk((ROWS, COLS), torch.uint8), mk((ROWS, COLS), torch.uint8)
        inps, isources = like(), mk((ROWS, COLS), torch.uint8)
        p = lambda xs: [x.data_ptr() for x in xs]
        torch.cuda.synchronize()
        s.set_flow_batch(BATCH)
        head = (p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks), p(crops), p(cmasks), p(blends), p(bmasks), p(bsources))
        kw = dict(d_crop_sources=p(csources), max_empty=npix // 100, margin=1, d_sources=p(sources), fill_radius=RADIUS, trials=50, tol=0.05, blend_feather=FEATHER)
        blendv = lambda: s.stabilize_video_blended_dev(*head, **kw)
        inpv = lambda: s.stabilize_video_inpainted_dev(*head, p(inps), p(isources), **kw)
        for _ in range(args.warmup):
            blendv(), s.synchronize(), inpv(), s.synchronize()
        te, tf = [], []
        res = None
        for _ in range(args.clip_reps):
            for fn, acc in ((blendv, te), (inpv, tf)):
                e0, e1 = event_pair()
                e0.record(stream)
                res = fn()
                s.synchronize()
                e1.record(stream)
                e1.synchronize()
                acc.append(e0.elapsed_time(e1) / PAIRS)
        e, f = float(np.median(te)), float(np.median(tf))
        ic = res["inpaint_counts"]
        print(json.dumps(dict(what="clip", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, batch=BATCH, radius=RADIUS, feather=FEATHER, reps=args.clip_reps,
                              window=list(res["window"]), e_blended_video_ms_per_pair=round(e, 3), e_min_max_ms=[round(min(te), 3), round(max(te), 3)],
                              f_inpainted_video_ms_per_pair=round(f, 3), f_min_max_ms=[round(min(tf), 3), round(max(tf), 3)],
                              f_minus_e_us_per_pair=round((f - e) * 1e3, 1), f_minus_e_percent_of_e=round(100.0 * (f - e) / e, 2),
                              e_spread_percent=round(100.0 * (max(te) - min(te)) / e, 2), f_within_e_spread=bool((f - e) <= (max(te) - min(te))),
                              inpainted_mean_share=round(float(ic.mean()) / npix, 5), inpainted_min_max=[int(ic.min()), int(ic.max())])), flush=True)


if __name__ == "__main__":
    main()
