"""Timing of the sharpen stage at 1280x720, BGR and gray ("Sharpen"), one process, HIP events on the context's stream, medians
of 20 repeated, warmed-up calls (tools/noise_curve_time.py's protocol); the variants of a group alternate, so that all see the same machine:

  (a) rsdsfm_sharpen_dev and rsdsfm_sharpen_curve_dev, each with and without the counters (the counters cost a memset node in front of the
      launch), on a textured frame under noise +-2 .. +-20 with a full mask;
  (b) beside them rsdsfm_denoise_spatial_dev at search 1 with every pixel deficient, with and without its counters -- the nearest existing kernel
      of the same tile and traffic, CH + 1 bytes in and CH out per pixel -- and a device-to-device copy of the image (CH bytes in, CH out) and of
      the image and the mask (CH + 1 in, CH + 1 out) as the floor;
  (c) rsdsfm_sharpen_dev with amount_q4 = 0 and under an empty mask: the workgroup-uniform early exit;
  (d) rsdsfm_sharpen_frame_dev against its parts, rsdsfm_noise_curve_dev and rsdsfm_sharpen_curve_dev, called one after another.

The expectation, stated before the run.  Nothing about this kernel has been measured.  It moves 2 CH + 1 bytes per pixel (6.45 MB BGR, 2.76 MB
gray), stages 5.6 KB per workgroup in LDS once and reads ten dwords per pixel from it; its arithmetic is some forty multiply-adds and CH exact
divisions per pixel, far less than the top-up's nine patch distances at search 1.  So it should be memory-bound: WITHOUT the counters nearer
the copy of image and mask than the top-up at search 1 without its counters.  profiles/denoise_spatial_time.txt has the top-up's early exit at
6.7 us without and 23.2 us with its counters: the memset node costs about 16 us in an event pair, and the same is expected here.  The curve form
forms a 256-entry table per workgroup: within 3 us of the fixed form.  The frame call enqueues what its parts enqueue: within 5 us of their sum.
No time is gated.  Every line says what came out, and the last says whether the expectation held.  One JSON line per measurement; the record is
profiles/sharpen_time.txt.

    python tools/sharpen_time.py [--reps 20] [--warmup 3] > profiles/sharpen_time.txt
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS, COLS = 720, 1280
NOISE = (2, 20)  # signal-dependent: the amplitude at byte 0 and at byte 255


def frame(channels, seed=5):
    """a textured frame whose levels cross every band, under noise that grows with the level"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:ROWS, 0:COLS]
    base = 20 + (215 * x) // (COLS - 1) + 12 * (2 * ((x // 8 + y // 8) % 2) - 1)
    base = np.stack([base] * channels, axis=-1).astype(np.int64)
    amp = NOISE[0] + ((NOISE[1] - NOISE[0]) * base + 127) // 255
    f = np.clip(base + rng.integers(-amp, amp + 1), 0, 255).astype(np.uint8)
    return f[..., 0] if channels == 1 else f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch

    import rsdsfm
    import rsdsfm_noise_curve as nc
    import rsdsfm_sharpen as sh

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
    with torch.cuda.device(dev), torch.cuda.stream(stream), rsdsfm.Solver(0, stream=stream.cuda_stream) as s:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        for ch in (3, 1):
            d_img, d_full, d_empty = up(frame(ch)), up(np.ones((ROWS, COLS), dtype=np.uint8)), up(np.zeros((ROWS, COLS), dtype=np.uint8))
            d_out, d_sup, d_mcopy = torch.empty_like(d_img), torch.empty_like(d_full), torch.empty_like(d_full)
            d_cnt, d_cnt3 = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
            d_hist, d_curve = torch.empty(8192, dtype=torch.int32, device=dev), torch.empty(36, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            I, M, O = d_img.data_ptr(), d_full.data_ptr(), d_out.data_ptr()
            nc.noise_curve_dev(s, I, M, ch, ROWS, COLS, d_hist.data_ptr(), d_curve.data_ptr())
            s.synchronize()
            lut = nc.noise_curve_strengths(d_curve.cpu().numpy().view(np.uint64).reshape(9, 4))
            fixed = lambda cnt, mask=M, amount=16: (lambda: sh.sharpen_dev(s, I, mask, ch, ROWS, COLS, O, cnt, amount))
            curve = lambda cnt: (lambda: sh.sharpen_curve_dev(s, I, M, ch, ROWS, COLS, d_curve.data_ptr(), O, cnt))
            top_up = lambda cnt: (lambda: s.denoise_spatial_dev(I, M, None, ch, ROWS, COLS, O, None, cnt, 12, 80, 1))

            def copy_image():
                d_out.copy_(d_img)

            def copy_both():
                d_out.copy_(d_img)
                d_mcopy.copy_(d_full)

            def parts():
                nc.noise_curve_dev(s, I, M, ch, ROWS, COLS, d_hist.data_ptr(), d_curve.data_ptr())
                sh.sharpen_curve_dev(s, I, M, ch, ROWS, COLS, d_curve.data_ptr(), O, d_cnt.data_ptr())

            calls = {"sharpen": fixed(None), "sharpen counted": fixed(d_cnt.data_ptr()), "sharpen curve": curve(None), "sharpen curve counted": curve(d_cnt.data_ptr()),
                     "top-up search 1": top_up(None), "top-up search 1 counted": top_up(d_cnt3.data_ptr()), "copy image": copy_image, "copy image and mask": copy_both,
                     "sharpen amount 0": fixed(None, amount=0), "sharpen empty mask": fixed(None, mask=d_empty.data_ptr()), "noise curve": lambda: nc.noise_curve_dev(
                         s, I, M, ch, ROWS, COLS, d_hist.data_ptr(), d_curve.data_ptr()), "frame parts": parts,
                     "frame": lambda: sh.sharpen_frame_dev(s, I, M, ch, ROWS, COLS, O, d_cnt.data_ptr(), d_curve.data_ptr())}
            ts = warmed(calls, s)
            fixed(d_cnt.data_ptr())()
            s.synchronize()
            counts = d_cnt.cpu().numpy().tolist()
            bytes_moved = (2 * ch + 1) * ROWS * COLS
            for name in calls:
                row = dict(what=name, size=size, channels=ch, reps=args.reps, us=med(ts[name]), min_max_us=mm(ts[name]))
                if name.startswith("sharpen") and "amount" not in name and "empty" not in name:
                    row.update(bytes=bytes_moved, gb_per_s=round(bytes_moved / float(np.median(ts[name])) / 1e3, 1))
                if name == "sharpen counted":
                    row.update(launches=sh.sharpen_launches(), counts_unset_kept_sharpened_limited=counts, strength_min_max=[int(lut.min()), int(lut.max())])
                if name == "frame":
                    row.update(launches=sh.sharpen_frame_launches())
                print(json.dumps(row), flush=True)
            m = {k_: float(np.median(v)) for k_, v in ts.items()}
            tag = "bgr" if ch == 3 else "gray"
            held["%s: nearer the copy than the top-up" % tag] = m["sharpen"] - m["copy image and mask"] < m["top-up search 1"] - m["sharpen"]
            held["%s: the curve form within 3 us" % tag] = abs(m["sharpen curve"] - m["sharpen"]) <= 3.0
            held["%s: the frame call within 5 us of its parts" % tag] = abs(m["frame"] - m["frame parts"]) <= 5.0
            print(json.dumps(dict(what="differences", channels=ch, sharpen_minus_copy_us=round(m["sharpen"] - m["copy image and mask"], 1),
                                  top_up_minus_sharpen_us=round(m["top-up search 1"] - m["sharpen"], 1), counters_us=round(m["sharpen counted"] - m["sharpen"], 1),
                                  curve_minus_fixed_us=round(m["sharpen curve"] - m["sharpen"], 1), frame_minus_parts_us=round(m["frame"] - m["frame parts"], 1))), flush=True)
        print(json.dumps(dict(what="expectation: without the counters the kernel lies nearer the copy of image and mask than the top-up at search 1, the curve form within 3 us "
                                   "of the fixed form, the frame call within 5 us of its parts", held=held, all_held=all(held.values()))), flush=True)


if __name__ == "__main__":
    main()
