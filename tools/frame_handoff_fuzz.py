"""Randomised campaign on the frame solve's hand-off from the RANSAC's winner to the refinement (rsdsfm_set_frame_handoff), GPU only: mode 0
(the first refinement pass gathers its inliers from the final stage's block-local lists) must return the bytes of mode 1 (the compaction
launch) -- result struct, depth map, pose table and the first m refined inliers, pixel indices and scanlines.  Two contexts, one per mode,
solve the same random frames in the same order (tests/fuzz_frames.py pins the refinement to the iterate-by-iterate arithmetic and so never
takes the direct form; this campaign runs the default arithmetic): small frames, DeepFlow-like and noise-free, holes of zero flow, random
motions, trial counts, tolerances from selective to permissive, acceleration mode, both flow index modes.
    usage (GPU box): python tools/frame_handoff_fuzz.py [cases] [seed]        (exit code 1 on a mismatch)"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch

    import rsdsfm

    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    dev = torch.device("cuda", 0)
    hip = ctypes.CDLL("libamdhip64.so")

    def d2h(ptr, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        if nbytes:
            assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 2) == 0
        return out.tobytes()

    bad = ran = partial = 0
    with rsdsfm.Solver(0) as s0, rsdsfm.Solver(0) as s1:
        s0.set_frame_handoff(0)
        s1.set_frame_handoff(1)
        for c in range(cases):
            rng = np.random.default_rng(seed0 * 1000003 + c)
            rows, cols = int(rng.integers(12, 160)), int(rng.integers(12, 200))
            cfg = int(rng.choice([1, 3, 3, 3]))
            v = rng.normal(size=3) * np.array([0.03, 0.03, 0.02])
            w = rng.normal(size=3) * 0.004
            k = float(rng.choice([0.0, 0.0, rng.uniform(-0.5, 0.8)]))
            d = rsdsfm.synth.make_config(cfg, seed=int(rng.integers(1 << 30)), v=v, w=w, k=k, rows=rows, cols=cols)
            img_h = d["flow_img"].copy()
            if rng.random() < 0.25:  # a hole of zero flow: the dense speculation fails
                r0, c0 = int(rng.integers(0, rows - 4)), int(rng.integers(0, cols - 4))
                img_h[r0:r0 + int(rng.integers(1, 12)), c0:c0 + int(rng.integers(1, 12))] = 0.0
            if not np.all(np.isfinite(img_h)) or int(np.count_nonzero(np.abs(img_h).sum(axis=2) > 1e-10)) < 9:
                continue
            kw = dict(trials=int(rng.integers(1, 24)), tol=float(rng.choice([0.0005, 0.002, 0.01, 0.05])), seed=int(rng.integers(1, 1 << 20)),
                      use_acceleration_mode=bool(rng.random() < 0.2), flow_index_mode=int(rng.choice([rsdsfm.FLOW_COMPAT_RANK, rsdsfm.FLOW_GATHERED])))
            img = torch.from_numpy(np.ascontiguousarray(img_h)).to(dev)
            recs = []
            for s in (s0, s1):
                dm = torch.full((cols, rows), -7.0, dtype=torch.float64, device=dev)
                R = torch.full((rows, 9), -7.0, dtype=torch.float64, device=dev)
                t = torch.full((rows, 3), -7.0, dtype=torch.float64, device=dev)
                try:
                    r = s.solve_frame_dev(img.data_ptr(), rows, cols, d["K"], d["gamma"], dm.data_ptr(), R.data_ptr(), t.data_ptr(), **kw)
                except rsdsfm.RsdsfmError as e:
                    recs.append(("error", str(e)))
                    continue
                s.synchronize()
                m = int(r["num_inliers"])
                recs.append((int(r["n"]), m, int(r["best_trial"]), bool(r["flipped"]), r["v"].tobytes(), r["w"].tobytes(), np.float64(r["k"]).tobytes(),
                             tuple(sorted((kk, np.float64(vv).tobytes()) for kk, vv in r["refine_summary"].items())), dm.cpu().numpy().tobytes(),
                             R.cpu().numpy().tobytes(), t.cpu().numpy().tobytes(), d2h(r["d_inliers"], 24 * m), d2h(r["d_inlier_idx"], 8 * m), d2h(r["d_scanline"], 4 * m)))
            ran += 1
            if recs[0][0] != "error" and 0 < recs[0][1] < recs[0][0]:
                partial += 1
            if recs[0] != recs[1]:
                bad += 1
                which = [i for i, (x, y) in enumerate(zip(recs[0], recs[1])) if x != y] if len(recs[0]) == len(recs[1]) else "shape"
                print("MISMATCH case %d (%dx%d, %s): fields %s" % (c, cols, rows, kw, which), flush=True)
    print("frame_handoff_fuzz: %d cases ran, %d mismatches; %d solves kept only a part of their points" % (ran, bad, partial))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
