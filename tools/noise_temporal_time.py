"""Timing of the temporal noise curve at 1280x720, BGR and gray ("Temporal noise curve"), one process, HIP events on the
context's stream, medians of 20 repeated, warmed-up calls (tools/noise_curve_time.py's protocol); the variants of a group alternate, so that all
see the same machine.  The scene is the denoise's noisy shift scene at this size: five frames of a periodic random texture (period 16 columns,
bytes 32 .. 223) that moves on by 8 columns per frame under uniform noise +-6, constant depth 4, identity pose tables, K = (32, 32, cx, cy), the
camera one unit further per frame -- so every neighbour registers exactly and the overlap is the frame less 8 or 16 columns.

  (a) rsdsfm_noise_pair_hist_dev on the own frame and its registered next neighbour (first = 1: the memset node and one launch) beside
      rsdsfm_noise_curve_dev on the own frame (a memset node and two launches) and rsdsfm_noise_curve_resolve_dev alone, so that
      noise curve - resolve is that call's memset and histogram launch;
  (b) rsdsfm_denoise_temporal_frame_dev at radius 2 (five sources) beside rsdsfm_denoise_curve_frame_dev on the same sources, without and with
      the top-up.

The expectation, stated before the run.  Nothing about this kernel has been measured.  The pair histogram reads 2 (CH + 1) bytes per pixel
(7.4 MB BGR, 3.7 MB gray) where the noise curve's histogram reads CH + 1, but does far less arithmetic per sample (one patch sum, one key per
pixel, where that kernel forms CH keys from a separable mask), and its flush is the same: every thread of a workgroup reads 32 words of the
table and adds the non-zero ones to the global histogram.  On a noisy frame the flush and the LDS atomics, not the reads, are expected to
dominate both, so the pair histogram should lie within 8 us of (noise curve - resolve) in the same run.  The frame call at radius 2 trades the
curve frame call's memset node and two launches (profiles/noise_curve_time.txt: about 22 us as a call of its own) for one memset node, four
pair histograms and one resolve: it is expected SLOWER, by three pair histograms or so -- between 20 and 90 us -- and the same with the top-up.
No time is gated.  Every line says what came out, and the last says whether the expectation held.  One JSON line per measurement; the record is
profiles/noise_temporal_time.txt.

    python tools/noise_temporal_time.py [--reps 20] [--warmup 3] > profiles/noise_temporal_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS = 720, 1280
FRAMES, SHIFT, NOISE, RADIUS = 5, 8, 6, 2
K = (32.0, 32.0, COLS / 2.0, ROWS / 2.0)


def shift_frames(channels, seed=7):
    base = np.random.default_rng(2441).integers(32, 224, size=(ROWS, 16, 3), dtype=np.uint8)
    rng = np.random.default_rng(7000 + seed)
    out = []
    for n in range(FRAMES):
        f = base[:, (np.arange(COLS) + SHIFT * n) % 16]
        f = np.ascontiguousarray(f[..., 1]) if channels == 1 else f
        out.append((f.astype(np.int64) + rng.integers(-NOISE, NOISE + 1, size=f.shape)).astype(np.uint8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    import rsdsfm
    import rsdsfm_noise_curve as nc
    import rsdsfm_noise_temporal as nt

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)

    def event_pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(calls, reps):
        """calls: name -> function; every repetition runs each once, in turn -> name -> list of microseconds"""
        ts = {k_: [] for k_ in calls}
        for _ in range(reps):
            for name, fn in calls.items():
                e0, e1 = event_pair()
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1) * 1e3)
        return ts

    def warmed(calls, s):
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
        s.synchronize()
        return timed(calls, args.reps)

    med = lambda v: round(float(np.median(v)), 1)
    mm = lambda v: [round(min(v), 1), round(max(v), 1)]
    size = "%dx%d" % (COLS, ROWS)
    held = {}
    A = np.stack([np.eye(3)] * FRAMES)
    c = np.array([[n * SHIFT * 4.0 / 32.0, 0.0, 0.0] for n in range(FRAMES)])
    scales = np.ones(FRAMES)
    q = FRAMES // 2
    _, _, M0, m0, _, _ = rsdsfm.retime_poses(A, c, A, c, scales, float(q), nsources=FRAMES)
    nb, _, Mn, mn = rsdsfm.neighbour_poses(A, c, A, c, scales, q, RADIUS)
    src = [q] + [int(n) for n in nb]
    M, m = np.concatenate([M0, Mn]), np.concatenate([m0, mn])
    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        u8 = lambda: torch.empty((ROWS, COLS), dtype=torch.uint8, device=dev)
        for ch in (3, 1):
            frames = shift_frames(ch)
            d_frames = [up(f) for f in frames]
            d_map = up(np.full((COLS, ROWS), 4.0))  # column-major
            d_R, d_t = up(np.tile(np.eye(3).reshape(1, 9), (ROWS, 1))), up(np.zeros((ROWS, 3)))
            # (a) the own frame and its next neighbour registered by hand: frame q + 1 shows SHIFT columns on in frame q's camera
            layer, lmask = np.zeros_like(frames[q]), np.zeros((ROWS, COLS), dtype=np.uint8)
            layer[:, SHIFT:], lmask[:, SHIFT:] = frames[q + 1][:, :COLS - SHIFT], 1
            d_ref, d_full, d_layer, d_lmask = d_frames[q], up(np.ones((ROWS, COLS), dtype=np.uint8)), up(layer), up(lmask)
            d_hist, d_curve = torch.empty(8192, dtype=torch.int32, device=dev), torch.empty(36, dtype=torch.int64, device=dev)
            d_hist2, d_curve2 = torch.empty(8192, dtype=torch.int32, device=dev), torch.empty(36, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            pair = lambda: nt.noise_pair_hist_dev(s, d_ref.data_ptr(), d_full.data_ptr(), d_layer.data_ptr(), d_lmask.data_ptr(), ch, ROWS, COLS, d_hist.data_ptr(), True)
            resolve = lambda: nt.noise_curve_resolve_dev(s, d_hist.data_ptr(), d_curve.data_ptr())
            spatial = lambda: nc.noise_curve_dev(s, d_ref.data_ptr(), d_full.data_ptr(), ch, ROWS, COLS, d_hist2.data_ptr(), d_curve2.data_ptr())
            pair()
            ts = warmed({"pair histogram": pair, "resolve": resolve, "noise curve": spatial}, s)
            pair(), resolve(), spatial()
            s.synchronize()
            cv, cs = d_curve.cpu().numpy().reshape(9, 4), d_curve2.cpu().numpy().reshape(9, 4)
            t = {k_: float(np.median(v)) for k_, v in ts.items()}
            diff = t["pair histogram"] - (t["noise curve"] - t["resolve"])
            tag = "bgr" if ch == 3 else "gray"
            held["%s: the pair histogram within 8 us of the noise curve's memset and histogram" % tag] = abs(diff) <= 8.0
            nbytes = 2 * (ch + 1) * ROWS * COLS
            print(json.dumps(dict(what="pair histogram beside the noise curve", size=size, channels=ch, reps=args.reps, launches=nt.noise_pair_hist_launches(),
                                  pair_hist_us=med(ts["pair histogram"]), pair_hist_min_max_us=mm(ts["pair histogram"]), resolve_us=med(ts["resolve"]),
                                  resolve_min_max_us=mm(ts["resolve"]), noise_curve_us=med(ts["noise curve"]), noise_curve_min_max_us=mm(ts["noise curve"]),
                                  pair_minus_curve_less_resolve_us=round(diff, 1), bytes=nbytes, gb_per_s=round(nbytes / t["pair histogram"] / 1e3, 1),
                                  temporal_n_m_sigma=[int(cv[8, 0]), int(cv[8, 1]), round(int(cv[8, 2]) / 256.0, 2)],
                                  spatial_n_m_sigma=[int(cs[8, 0]), int(cs[8, 1]), round(int(cs[8, 2]) / 256.0, 2)],
                                  sigma_true=round(float(np.sqrt(((2 * NOISE + 1) ** 2 - 1) / 12.0)), 2))), flush=True)
            # (b) the frame calls on the same five sources
            pick = lambda xs: [xs[n].data_ptr() for n in src]
            same = lambda x: [x.data_ptr()] * len(src)
            out, t_mask, t_w, sup = torch.empty_like(d_frames[0]), u8(), u8(), u8()
            counts6 = torch.zeros(6, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            fargs = (pick(d_frames), ch, same(d_map), same(d_R), same(d_t), K, ROWS, COLS, M, m, out.data_ptr(), t_mask.data_ptr(), t_w.data_ptr())
            calls = dict(curve=lambda: nc.denoise_curve_frame_dev(s, *fargs, None, counts6.data_ptr(), d_curve2.data_ptr()),
                         temporal=lambda: nt.denoise_temporal_frame_dev(s, *fargs, None, counts6.data_ptr(), d_curve.data_ptr()),
                         curve_both=lambda: nc.denoise_curve_frame_dev(s, *fargs, sup.data_ptr(), counts6.data_ptr(), d_curve2.data_ptr(), spatial=True),
                         temporal_both=lambda: nt.denoise_temporal_frame_dev(s, *fargs, sup.data_ptr(), counts6.data_ptr(), d_curve.data_ptr(), spatial=True))
            tf = warmed(calls, s)
            calls["temporal"](), calls["curve"]()
            s.synchronize()
            cv, cs = d_curve.cpu().numpy().reshape(9, 4), d_curve2.cpu().numpy().reshape(9, 4)
            lut_t, lut_s = nc.noise_curve_strengths(cv.view(np.uint64)), nc.noise_curve_strengths(cs.view(np.uint64))
            d1 = float(np.median(tf["temporal"])) - float(np.median(tf["curve"]))
            d2 = float(np.median(tf["temporal_both"])) - float(np.median(tf["curve_both"]))
            held["%s: the frame call 20 to 90 us slower" % tag] = 20.0 <= d1 <= 90.0
            held["%s: the frame call with the top-up 20 to 90 us slower" % tag] = 20.0 <= d2 <= 90.0
            print(json.dumps(dict(what="frame %d at radius %d, %d sources" % (q, RADIUS, len(src)), size=size, channels=ch, reps=args.reps,
                                  launches=dict(curve=nc.denoise_curve_frame_launches(ROWS, COLS, len(src)), temporal=nt.denoise_temporal_frame_launches(ROWS, COLS, len(src)),
                                                temporal_both=nt.denoise_temporal_frame_launches(ROWS, COLS, len(src), True)),
                                  denoise_curve_frame_us=med(tf["curve"]), denoise_curve_frame_min_max_us=mm(tf["curve"]), denoise_temporal_frame_us=med(tf["temporal"]),
                                  denoise_temporal_frame_min_max_us=mm(tf["temporal"]), difference_us=round(d1, 1), denoise_curve_frame_with_top_up_us=med(tf["curve_both"]),
                                  denoise_curve_frame_with_top_up_min_max_us=mm(tf["curve_both"]), denoise_temporal_frame_with_top_up_us=med(tf["temporal_both"]),
                                  denoise_temporal_frame_with_top_up_min_max_us=mm(tf["temporal_both"]), difference_with_top_up_us=round(d2, 1),
                                  temporal_n_m=[int(cv[8, 0]), int(cv[8, 1])], temporal_strength_min_max=[int(lut_t.min()), int(lut_t.max())],
                                  spatial_n_m=[int(cs[8, 0]), int(cs[8, 1])], spatial_strength_min_max=[int(lut_s.min()), int(lut_s.max())],
                                  counts6=counts6.cpu().numpy().tolist())), flush=True)
        print(json.dumps(dict(what="expectation: the pair histogram within 8 us of the noise curve's memset and histogram launch; the temporal frame call at radius 2 between 20 and "
                                   "90 us slower than the curve frame call, without and with the top-up", held=held, all_held=all(held.values()))), flush=True)


if __name__ == "__main__":
    main()
