"""Writes tests/golden/golden_stabilize_blend_v1.npz: inputs and outputs of the seam blend's definition (tests/stabilize_blend_spec_numpy.py)
-- the distance planes of random masks, and frames of tests/stabilize_fill_cases.clip_case blended through the windows of the crop's fixture
(tests/golden/golden_stabilize_crop_v1.npz): (33, 70) BGR, frame 1 at radius 2, feather 4; (24, 40) gray, frame 3 at radius 1, feather 16,
the gain off; (33, 70) gray, frame 2 at radius 2 through the FULL frame, feather 16 -- tests/test_stabilize_blend_cpu.py recomputes them.  Run from the repository root:
    python tests/golden/make_golden_stabilize_blend.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import stabilize_blend_cases as cases  # noqa: E402
import stabilize_blend_spec_numpy as spec  # noqa: E402

# (rows, cols, channels, frame q, radius, mode, q5_mode, iterations, feather, min_overlap, gain_mode, the crop fixture's window or the frame)
CASES = [(33, 70, 3, 1, 2, 0, 0, 0, 4, 64, 0, True), (24, 40, 1, 3, 1, 0, 1, 2, 16, 32, 1, True), (33, 70, 1, 2, 2, 0, 0, 0, 16, 64, 0, False)]
# (rows, cols, empty, seed, feather)
MASKS = [(96, 128, 0.01, 1, 16), (33, 70, 0.02, 2, 64), (7, 5, 0.1, 3, 2)]


def main():
    crop = np.load(os.path.join(HERE, "golden_stabilize_crop_v1.npz"))
    out = {}
    for rows, cols, empty, seed, T in MASKS:
        m = cases.random_masks(rows, cols, 1, empty, seed)[0]
        n = "mask%dx%d/" % (rows, cols)
        out.update({n + "params": np.array([seed, T]), n + "empty": np.array(empty), n + "mask": np.packbits(m != 0), n + "dist": spec.seam_distance(m, T)})
    for rows, cols, ch, q, radius, mode, q5, it, T, min_overlap, gain_mode, cropped in CASES:
        cc = cases.clip_case(oracle_py.pose_table, rows, cols, channels=ch)
        window = tuple(int(x) for x in crop["%dx%d/window" % (rows, cols)]) if cropped else (0, 0, rows, cols)
        r = spec.blend_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], q, cc["M"][q], cc["m"][q],
                             window, radius=radius, T=T, min_overlap=min_overlap, gain_mode=gain_mode, mode=mode, q5_mode=q5, iterations=it)
        n = "%dx%dx%d/" % (rows, cols, ch)
        out.update({n + "modes": np.array([ch, q, radius, mode, q5, it, T, min_overlap, gain_mode]), n + "window": np.array(window), n + "out_image": r["image"],
                    n + "out_mask": r["mask"], n + "out_source": r["source"], n + "out_dist": r["dist"], n + "out_gains": r["gains"], n + "out_sums": r["sums"],
                    n + "out_counts": np.array(r["counts"], dtype=np.int64)})
    path = os.path.join(HERE, "golden_stabilize_blend_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        if k.endswith("window") or k.endswith("out_counts") or k.endswith("out_gains"):
            print(k, out[k].tolist())


if __name__ == "__main__":
    main()
