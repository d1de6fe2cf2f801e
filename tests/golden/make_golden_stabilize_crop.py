"""Writes tests/golden/golden_stabilize_crop_v1.npz: inputs and outputs of the crop's definition (tests/stabilize_crop_spec_numpy.py) -- the
window of random masks, and frames of tests/stabilize_fill_cases.clip_case through the window of their clip's filled masks: (33, 70) BGR,
frame 1 at radius 2; (24, 40) gray, frame 3 at radius 1; (5, 3) BGR, frame 2 at radius 0 -- tests/test_stabilize_crop_cpu.py recomputes
them.  Run from the repository root:
    python tests/golden/make_golden_stabilize_crop.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import oracle_py  # noqa: E402
import stabilize_crop_cases as cases  # noqa: E402
import stabilize_crop_spec_numpy as spec  # noqa: E402
import stabilize_fill_spec_numpy as fill  # noqa: E402

# (rows, cols, channels, frame q, radius, mode, q5_mode, iterations, margin)
CASES = [(33, 70, 3, 1, 2, 0, 0, 0, 1), (24, 40, 1, 3, 1, 0, 1, 2, 0), (5, 3, 3, 2, 0, 1, 0, 3, 0)]
# (rows, cols, planes, empty, seed, max_empty, margin)
MASKS = [(96, 128, 5, 0.01, 1, 0, 1), (33, 70, 3, 0.02, 2, 2, 0), (7, 5, 1, 0.1, 3, 0, 3)]


def clip_masks(cc, radius, mode, q5, it):
    """the masks the inner clip call writes: every frame's filled mask (radius 0: its own)"""
    out = []
    for q in range(len(cc["depths"])):
        if radius:
            r = fill.stabilize_filled_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], q, cc["M"][q],
                                            cc["m"][q], radius=radius, mode=mode, q5_mode=q5, iterations=it)
        else:
            r = fill.stab.stabilize_frame(cc["images"][q], cc["depths"][q], cc["Rs"][q], cc["ts"][q], cc["K"], cc["M"][q], cc["m"][q], mode=mode, q5_mode=q5,
                                          iterations=it)
        out.append(r["mask"])
    return np.stack(out)


def main():
    out = {}
    for rows, cols, planes, empty, seed, max_empty, margin in MASKS:
        m = cases.random_masks(rows, cols, planes, empty, seed)
        n = "mask%dx%d/" % (rows, cols)
        out.update({n + "params": np.array([planes, seed, max_empty, margin]), n + "empty": np.array(empty), n + "masks": np.packbits(m != 0),
                    n + "window": np.array(spec.crop_window(m, max_empty, margin))})
    for rows, cols, ch, q, radius, mode, q5, it, margin in CASES:
        cc = cases.clip_case(oracle_py.pose_table, rows, cols, channels=ch)
        masks = clip_masks(cc, radius, mode, q5, it)
        window = spec.crop_window(masks, 0, margin)
        r = spec.stabilize_cropped_frame(cc["images"], cc["depths"], cc["Rs"], cc["ts"], cc["K"], cc["A"], cc["c"], cc["As"], cc["cs"], cc["scales"], q, cc["M"][q],
                                         cc["m"][q], window, radius=radius, mode=mode, q5_mode=q5, iterations=it)
        n = "%dx%d/" % (rows, cols)
        out.update({n + "modes": np.array([ch, q, radius, mode, q5, it, margin]), n + "masks": np.packbits(masks), n + "window": np.array(window),
                    n + "out_image": r["image"], n + "out_mask": r["mask"], n + "out_source": r["source"], n + "out_counts": np.array(r["counts"], dtype=np.int64)})
    path = os.path.join(HERE, "golden_stabilize_crop_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in sorted(out):
        if k.endswith("window") or k.endswith("out_counts"):
            print(k, out[k].tolist())


if __name__ == "__main__":
    main()
