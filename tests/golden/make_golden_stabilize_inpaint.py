"""Writes tests/golden/golden_stabilize_inpaint_v1.npz: outputs of the inpainting's definition (tests/stabilize_inpaint_spec_numpy.py) on
inputs that tests/stabilize_inpaint_cases.py makes again from a seed -- (33, 70) BGR under the bands mask, (129, 67) gray under the random
mask, (7, 5) BGR with only the last pixel set -- tests/test_stabilize_inpaint_cpu.py recomputes them.  Run from the repository root:
    python tests/golden/make_golden_stabilize_inpaint.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import stabilize_inpaint_cases as cases  # noqa: E402
import stabilize_inpaint_spec_numpy as spec  # noqa: E402

# (rows, cols, channels, seed, index into cases.masks)
CASES = [(33, 70, 3, 5, 3), (129, 67, 1, 6, 4), (7, 5, 3, 7, 2)]


def main():
    out = {}
    for rows, cols, ch, seed, family in CASES:
        image, (name, mask) = cases.image_of(rows, cols, ch, seed), cases.masks(rows, cols, seed)[family]
        source = np.zeros((rows, cols), dtype=np.uint8)
        count = spec.inpaint(image, mask, source)
        n = "%dx%dx%d/" % (rows, cols, ch)
        out.update({n + "params": np.array([seed, family]), n + "mask": np.packbits(mask != 0), n + "out_image": image, n + "out_source": np.packbits(source != 0),
                    n + "out_count": np.array(count, dtype=np.int64)})
        print(n, name, "count", count)
    path = os.path.join(HERE, "golden_stabilize_inpaint_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
