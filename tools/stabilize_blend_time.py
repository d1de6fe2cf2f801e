"""Timing of the stabiliser's seam blend at 1280x720 ("Seam blend"), one process, HIP events on the context's stream,
medians over repeated, warmed-up calls:

  (a) rsdsfm_seam_distance_dev, feather 16, on a mask that is 99 % own (a band of 0.5 % of each side empty along two edges);
  (b) one rsdsfm_seam_blend_layer_dev, BGR, of a full layer onto that mask's planes (99 % own: the untouched path almost everywhere) and
  (c) onto empty planes (every pixel filled).  The in-out planes are restored before every timed call, outside the timed window; (a), (b)
      and (c) alternate, so that all see the same machine;
  (d) rsdsfm_stabilize_video_cropped_dev against (e) rsdsfm_stabilize_video_blended_dev at radius 2 over 16 pairs at B = 8, alternating, per
      pair, with the spread of the repetitions;
  (f) the seam step on an exposure clip: render_sequence(gains=...) with +-10 % between consecutive frames, 6 frames of 240 x 320, end to end
      through evaluate_real_sequence(stabilize=True, fill=2, blend=True): the mean absolute difference between horizontally and vertically
      adjacent pixels of which one is the own frame's and one a neighbour's (by the filled clip's source plane), in the filled and in the
      blended clip, the gains found against the gains applied, and what the solve made of the exposure change.
The expectations: the small launches are launch-bound, a few us each; (e) - (d) is one more own pass, a full render per
neighbour and 2 + 2 K small launches per pair, roughly what the crop added.  Every line says what came out.  One JSON line per measurement;
the record is profiles/stabilize_blend_time.txt.

    python tools/stabilize_blend_time.py [--reps 20] [--clip-reps 5] [--warmup 3] > profiles/stabilize_blend_time.txt
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


def seam_step(filled, blended, source):
    """mean |a - b| over adjacent pixel pairs (horizontal and vertical) with one pixel the own frame's (1) and one a neighbour's (>= 2)"""
    f, b = filled.astype(np.float64), blended.astype(np.float64)
    tot_f = tot_b = n = 0.0
    for ax in (0, 1):
        s0, s1 = (source[:-1], source[1:]) if ax == 0 else (source[:, :-1], source[:, 1:])
        sel = ((s0 == 1) & (s1 >= 2)) | ((s0 >= 2) & (s1 == 1))
        for img, which in ((f, 0), (b, 1)):
            d = np.abs(np.diff(img, axis=ax))
            d = d.mean(axis=2) if d.ndim == 3 else d
            if which == 0:
                tot_f += d[sel].sum()
            else:
                tot_b += d[sel].sum()
        n += sel.sum()
    return (tot_f / n, tot_b / n, int(n)) if n else (0.0, 0.0, 0)


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
        empty = torch.zeros_like(own)
        image0, layer = torch.from_numpy(frames[0]).to(dev), torch.from_numpy(frames[1]).to(dev)
        lmask = torch.ones_like(own)
        dist_own, dist_empty = torch.empty_like(own), torch.empty_like(own)
        image, mask, source = torch.empty_like(image0), torch.empty_like(own), torch.empty_like(own)
        rec, cnt = torch.zeros(8, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        s.seam_distance_dev(own.data_ptr(), ROWS, COLS, FEATHER, dist_own.data_ptr())
        s.seam_distance_dev(empty.data_ptr(), ROWS, COLS, FEATHER, dist_empty.data_ptr())
        s.synchronize()

        def restore(start):  # on the solver's stream (torch's current stream here), in front of the timed window
            if start is not None:
                image.copy_(image0), mask.copy_(start), source.copy_(start)

        dist_call = lambda: s.seam_distance_dev(own.data_ptr(), ROWS, COLS, FEATHER, dist_empty.data_ptr())
        blend = lambda d: (lambda: s.seam_blend_layer_dev(layer.data_ptr(), lmask.data_ptr(), 3, ROWS, COLS, d.data_ptr(), 2, image.data_ptr(), mask.data_ptr(),
                                                          source.data_ptr(), rec.data_ptr(), cnt.data_ptr(), feather=FEATHER))
        dist_zero = torch.zeros_like(own)
        calls = dict(a=(None, dist_call), b=(own, blend(dist_own)), c=(empty, blend(dist_zero)))
        for start, fn in calls.values():
            for _ in range(args.warmup):
                restore(start), fn()
        s.synchronize()
        ts, counts = dict(a=[], b=[], c=[]), {}
        for _ in range(args.reps):
            for name, (start, fn) in calls.items():
                restore(start)
                e0, e1 = event_pair()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3)
                counts[name] = cnt.cpu().numpy().tolist()
        med = {k_: float(np.median(v_)) for k_, v_ in ts.items()}
        mm = lambda k_: [round(min(ts[k_]), 1), round(max(ts[k_]), 1)]
        print(json.dumps(dict(what="frame", size="%dx%d" % (COLS, ROWS), feather=FEATHER, reps=args.reps, own_share=round(float(own.sum().cpu()) / npix, 4),
                              launches=dict(a=rsdsfm.seam_distance_launches(ROWS, COLS), b=rsdsfm.seam_blend_layer_launches(ROWS, COLS)),
                              a_seam_distance_us=round(med["a"], 1), a_min_max_us=mm("a"), b_blend_layer_own99_us=round(med["b"], 1), b_min_max_us=mm("b"),
                              c_blend_layer_empty_us=round(med["c"], 1), c_min_max_us=mm("c"), b_filled_blended=counts["b"], c_filled_blended=counts["c"])), flush=True)
        # the clip: (d) and (e) alternate
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
        head = (p(d_frames), ROWS, COLS, 3, K, 0.8, p(dms), p(flows), p(Rs), p(Ts), p(stabs), p(smasks), p(crops), p(cmasks))
        kw = dict(d_crop_sources=p(csources), max_empty=npix // 100, margin=1, d_sources=p(sources), fill_radius=RADIUS, trials=50, tol=0.05)
        cropv = lambda: s.stabilize_video_cropped_dev(*head, **kw)
        blendv = lambda: s.stabilize_video_blended_dev(*head, p(blends), p(bmasks), p(bsources), blend_feather=FEATHER, **kw)
        for _ in range(args.warmup):
            cropv(), s.synchronize(), blendv(), s.synchronize()
        td, te = [], []
        res = None
        for _ in range(args.clip_reps):
            for fn, acc in ((cropv, td), (blendv, te)):
                e0, e1 = event_pair()
                e0.record(stream)
                res = fn()
                s.synchronize()
                e1.record(stream)
                e1.synchronize()
                acc.append(e0.elapsed_time(e1) / PAIRS)
        d, e = float(np.median(td)), float(np.median(te))
        layers = sum(len(rsdsfm.neighbour_poses(res["A"], res["c"], res["A_s"], res["c_s"], res["scales"], q, RADIUS)[0]) for q in range(PAIRS)) / PAIRS
        bc = res["blend_counts"]
        print(json.dumps(dict(what="clip", size="%dx%d" % (COLS, ROWS), pairs=PAIRS, batch=BATCH, radius=RADIUS, feather=FEATHER, reps=args.clip_reps,
                              window=list(res["window"]), d_cropped_video_ms_per_pair=round(d, 3), d_min_max_ms=[round(min(td), 3), round(max(td), 3)],
                              e_blended_video_ms_per_pair=round(e, 3), e_min_max_ms=[round(min(te), 3), round(max(te), 3)],
                              e_minus_d_us_per_pair=round((e - d) * 1e3, 1), layers_per_pair=round(layers, 2), renders_per_pair=round(1 + layers, 2),
                              small_launches_per_pair=round(2 + 2 * layers, 2), e_minus_d_percent_of_d=round(100.0 * (e - d) / d, 2),
                              d_spread_percent=round(100.0 * (max(td) - min(td)) / d, 2), e_within_d_spread=bool((e - d) <= (max(td) - min(td))),
                              blended_mean_share=round(float(bc[:, 3::2].sum(axis=1).mean()) / npix, 5), filled_mean_share=round(float(bc[:, 2::2].sum(axis=1).mean()) / npix, 5),
                              gains_min_max=[int(res["gains"].min()), int(res["gains"].max())])), flush=True)
    # (f) the seam step on the exposure clip, end to end
    rows, cols, gamma, nf = 240, 320, 0.8, 6
    K2 = (0.75 * cols, 0.75 * cols, 0.5 * cols, 0.5 * rows)
    v, w, k = rsdsfm.synth.default_motion()
    f0, _ = rsdsfm.synth.make_flow(rows, cols, K2, v, w, k, gamma, _model_only=True)
    sc = 3.0 / np.abs(f0).max()
    applied = [1.0, 1.1, 1.0, 0.9, 1.0, 1.1]
    speeds = (1.0, 1.4, 0.8, 1.0, 1.2)
    out = {}
    with rsdsfm.Solver(0) as s:
        for name, g in (("plain", None), ("exposure", applied)):
            fr, _, _ = rsdsfm.synth.render_sequence(nf, rows, cols, K2, v * sc, w * sc, k, gamma, seed=21, speeds=speeds, gains=g)
            out[name] = rsdsfm.evaluate.evaluate_real_sequence(s, fr, camera=K2, gamma=gamma, trials=50, seeds=[3 + 5 * i for i in range(nf - 1)], stabilize=True,
                                                               smooth_sigma=1.0, fill=RADIUS, blend=True)
    for name, r in out.items():
        steps = [seam_step(r["stab_filled"][q], r["stab_blended"][q], r["stab_sources"][q]) for q in range(nf - 1)]
        n = sum(x[2] for x in steps)
        line = dict(what="seam", clip=name, size="%dx%d" % (cols, rows), frames=nf, radius=RADIUS, feather=FEATHER, seam_pairs=n,
                    filled_mean_abs_step=round(sum(x[0] * x[2] for x in steps) / max(n, 1), 3), blended_mean_abs_step=round(sum(x[1] * x[2] for x in steps) / max(n, 1), 3),
                    inliers=[int(o["num_inliers"]) for o in r["pairs"]], scales=[round(float(x), 4) for x in r["scales"]],
                    blend_counts=r["blend_counts"].tolist())
        if name == "exposure":
            found, want = [], []
            for q in range(nf - 1):
                for fq, sid in zip(*rsdsfm.neighbour_poses(r["A"], r["c"], r["path_smoothed"]["A_s"], r["path_smoothed"]["c_s"], r["scales"], q, RADIUS)[:2]):
                    found.append(round(float(r["blend_gains"][q][int(sid) - 2].mean()) / 65536.0, 4))
                    want.append(round(applied[q] / applied[int(fq)], 4))
            line.update(gains_found=found, gains_applied=want, gain_max_rel_error=round(max(abs(a / b - 1.0) for a, b in zip(found, want)), 4))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
